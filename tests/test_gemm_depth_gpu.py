"""Depth-specialised decode GEMMs (csrc/gemm.hip: gemm_depth_kernel, gemm_gateup48_kernel) against the kernel they
replace.  -m gpu.

MTTS_GEMM_DEPTH=0 sends every GEMM through gemm_skinny_kernel.  Every output element keeps its sum tree (same wave, same k-tiles in the same order, same LDS reduction,
same split-K slabs; a column's value does not depend on the block that computes it), so everything here is compared
BITWISE between the switch on and off.  mtts_debug_gemm_depth_launches counts the launches that took a specialised
kernel, so every comparison also checks that the switch-on leg ran the new kernels and the switch-off leg did not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402

# the four projections of a layer at the bench's dims (hidden 2048, intermediate 6144, 16 / 8 heads of 128): (N, K)
QKV, O_PROJ, DOWN, GATE_UP = (4096, 2048), (2048, 2048), (2048, 6144), (12288, 2048)


def _inputs(M, N, K, seed):
    """bf16 operands with exact zeros (a whole zero row, zero columns, scattered zeros) and a few rows of large magnitude."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    w = 0.05 * torch.randn(N, K, device="cuda", generator=g)
    x = torch.randn(M, K, device="cuda", generator=g)
    w[torch.rand(N, K, device="cuda", generator=g) < 0.02] = 0.0
    x[torch.rand(M, K, device="cuda", generator=g) < 0.05] = 0.0
    w[7] = 0.0
    w[:, 33] = 0.0
    x[M // 2] = 0.0
    x[0] *= 3.0e4
    x[M - 1] *= -1.0e3
    w[N - 5] *= 2.0e3
    w[100] *= 5.0e2
    return w.to(torch.bfloat16).contiguous(), x.to(torch.bfloat16).contiguous()


def _count():
    return int(capi.lib().mtts_debug_gemm_depth_launches())


def _bits(t):
    return t.view(torch.int16).cpu().numpy()


@pytest.mark.parametrize("M", [32, 5])
@pytest.mark.parametrize("N,K", [QKV, O_PROJ, DOWN])
def test_partial_epilogue_bitwise(monkeypatch, M, N, K):
    """qkv / o_proj / down_proj (split-K slabs, 8 / 4 / 12 k-tiles per wave) at 32 rows and at 5.  (qkv has no
    specialised instantiation -- it did not win its timing -- and runs gemm_skinny_kernel either way.)"""
    lib = capi.lib()
    w, x = _inputs(M, N, K, 1000 + N // 32 + K + M)
    outs = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("MTTS_GEMM_DEPTH", sw)
        y = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
        c0 = _count()
        capi.check(lib.mtts_k_gemm_bf16(w.data_ptr(), x.data_ptr(), y.data_ptr(), M, N, K, 0, None))
        torch.cuda.synchronize()
        # o_proj and down_proj have a specialised kernel, qkv has none; the switch turns it off
        assert _count() - c0 == (1 if sw == "1" and (N, K) != QKV else 0)
        outs[sw] = _bits(y)
    assert np.array_equal(outs["1"], outs["0"])
    # and it is the product: fp32 reference at bf16 resolution
    ref = x.float() @ w.float().T
    got = torch.from_numpy(outs["1"]).cuda().view(torch.bfloat16).float()
    tol = 2.0 ** -7 * ref.abs() + 2e-3 * ref.abs().amax(dim=1, keepdim=True)
    assert bool(((got - ref).abs() <= tol).all())


@pytest.mark.parametrize("M", [32, 5])
def test_swiglu_epilogue_bitwise(monkeypatch, M):
    """gate/up on 256 blocks of 48 columns against 384 blocks of 32, through mtts_k_gemm_swiglu_bf16."""
    lib = capi.lib()
    N, K = GATE_UP
    w, x = _inputs(M, N, K, 77 + M)
    x[0] /= 3.0e4                                  # keep silu(gate) * up finite in most columns of the large rows
    outs = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("MTTS_GEMM_DEPTH", sw)
        y = torch.zeros(M, N // 2, dtype=torch.bfloat16, device="cuda")
        c0 = _count()
        capi.check(lib.mtts_k_gemm_swiglu_bf16(w.data_ptr(), x.data_ptr(), y.data_ptr(), M, N, K, None))
        torch.cuda.synchronize()
        assert _count() - c0 == (1 if sw == "1" else 0)
        outs[sw] = _bits(y)
    assert np.array_equal(outs["1"], outs["0"])
    assert np.count_nonzero(outs["1"]) > 0.5 * outs["1"].size
    # and it is SwiGLU of the interleaved rows, with the reference's bf16 rounding points
    r = lambda t: t.to(torch.bfloat16).float()
    z = r(x.float() @ w.float().T)
    gate, up = z[:, 0::2], z[:, 1::2]
    ref = r(r(gate * torch.sigmoid(gate)) * up)
    got = torch.from_numpy(outs["1"]).cuda().view(torch.bfloat16).float()
    fin = torch.isfinite(ref) & torch.isfinite(got)
    assert float(fin.float().mean()) > 0.99
    tol = 2.0 ** -5 * ref.abs() + 2e-2 * torch.where(fin, ref, torch.zeros_like(ref)).abs().amax(dim=1, keepdim=True)
    assert bool((((got - ref).abs() <= tol) | ~fin).all())


def _rand_weights(cfg, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    lo, hi = cfg["speech_token_range"]
    for name, shape, kind in synth.weight_shapes(cfg):
        if kind == "norm":
            t = (1.0 + 0.1 * torch.randn(shape, device="cuda", generator=g)).to(torch.bfloat16)
        else:
            t = (0.02 * torch.randn(shape, device="cuda", generator=g)).to(torch.bfloat16)
            if name.endswith("embedding_list.0.weight"):
                t[lo:hi] *= 8.0
        yield name, t


def _prompts(cfg, seed, lens):
    """One prompt of exactly each length in `lens`, left-padded into a batch."""
    seqs = [synth.synth_prompts(cfg, seed + i, 1, n, 0.4, False)[0][0] for i, n in enumerate(lens)]
    return synth.left_pad(seqs, cfg["pad_token_id"])


def _run(monkeypatch, cfg, sw, batches, plen, steps, max_seq_len):
    """batches: batch sizes (ragged prompts of up to plen tokens) or tuples of exact prompt lengths."""
    from mtts.engine import Engine
    monkeypatch.setenv("MTTS_GEMM_DEPTH", sw)
    monkeypatch.setenv("MTTS_GRAPHS", "1")
    sizes = [B if isinstance(B, int) else len(B) for B in batches]
    eng = Engine(cfg, max_batch=max(sizes), max_seq_len=max_seq_len)
    for name, t in _rand_weights(cfg, 5):
        eng.bind(name, t)
    layers = [dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.05)] * 8
    res = []
    for B in batches:
        ids, mask = synth.synth_prompts(cfg, 300 + B, B, plen, 0.4, True) if isinstance(B, int) else _prompts(cfg, 300, B)
        eng.begin(ids, mask, ids.shape[1] + steps + 8, layers=layers, do_samples=[True] * 8, seed=13)
        eng.step(steps)
        eng.sync_state()
        gen = eng.read_generated(steps + 8)
        l0, l17 = eng.read_logits()
        res.append((gen, l0.view(np.uint32), l17.view(np.uint32)))
    eng.close()
    return res


def _same(a, b, steps):
    for (ga, l0a, l17a), (gb, l0b, l17b) in zip(a, b):
        assert ga.shape == gb.shape and ga.shape[0] >= steps
        assert np.array_equal(ga, gb)
        assert np.array_equal(l0a, l0b) and np.array_equal(l17a, l17b)


def test_engine_bitwise_at_bench_width(monkeypatch):
    """Hidden 2048 / intermediate 6144 / 16 + 8 heads (three layers): batch 32 and batch 5, ragged prompts of up to 1200
    tokens = 19 KV pages, i.e. three pass-B chunks with a ragged last one for the long rows and fewer for the short
    ones; 24 sampled steps under graph replay.  Generated ids and the last step's logits, switch on against off."""
    cfg = synth.assumed_1p7b()
    cfg["num_hidden_layers"] = 3
    steps = 24
    c0 = _count()
    on = _run(monkeypatch, cfg, "1", (32, 5), 1200, steps, 1408)
    c1 = _count()
    off = _run(monkeypatch, cfg, "0", (32, 5), 1200, steps, 1408)
    # o_proj, gate/up and down_proj of each of the three layers, at least once per batch size (graphs: counted at capture)
    assert c1 - c0 >= 2 * 3 * 3 and _count() == c1
    _same(on, off, steps)


def test_engine_bitwise_at_bench_context(monkeypatch):
    """The bench's own context (one layer at its width, batch 5: the general path): prompts of 4300 / 4090 / 4000 / 3500 /
    600 tokens = 68 / 64 / 63 / 55 / 10 KV pages, i.e. 9, 8 (full: the boundary of the first group of 8 chunk
    partials; it becomes 9 when the row crosses 4096 during the run), 8 (ragged), 7 and 2 pass-B chunks: the decode
    chain around the GEMMs as the benchmark runs it."""
    cfg = synth.assumed_1p7b()
    cfg["num_hidden_layers"] = 1
    steps = 24
    lens = ((4300, 4090, 4000, 3500, 600),)
    c0 = _count()
    on = _run(monkeypatch, cfg, "1", lens, 0, steps, 4480)
    c1 = _count()
    off = _run(monkeypatch, cfg, "0", lens, 0, steps, 4480)
    assert c1 - c0 >= 3 and _count() == c1
    _same(on, off, steps)


def test_engine_tiny_dims_fall_back(monkeypatch):
    """Dims that no specialised instantiation fits (hidden 256: 2 k-tiles per wave): with the switch on every GEMM is
    the old kernel (no specialised launch is counted), and the run is the same as with the switch off."""
    cfg = synth.tiny()
    steps = 24
    c0 = _count()
    on = _run(monkeypatch, cfg, "1", (32, 5), 700, steps, 896)
    off = _run(monkeypatch, cfg, "0", (32, 5), 700, steps, 896)
    assert _count() == c0
    _same(on, off, steps)
