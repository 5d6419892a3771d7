"""The seam o_proj -> post-attention RMSNorm -> gate/up as two launches (csrc/gemm_fold.hip, MTTS_FOLD_NORM) against the
three launches it replaces.  -m gpu.  Nothing here has a tolerance: every comparison is bitwise.

The expected values are made by the launches the engine runs today, through their hooks:
  * o_proj: launch_gemm with the fp32-slab epilogue and split-K 4 (mtts_k_gemm_bf16 with ksplit = 4, MTTS_GEMM_DEPTH=1:
    gemm_depth_kernel<8, 4, 0>), whose slabs the hook sums in the order ((s0 + s1) + s2) + s3 and rounds to bf16 -- the
    first thing resid_norm_kernel does with them;
  * mtts_k_resid_norm on that bf16 Linear output as one fp32 slab (exact: bf16(bf16(y)) == bf16(y)), which gives x' and
    RMSNorm(x') * w;
  * mtts_k_gemm_swiglu_bf16 (gemm_gateup48_kernel<8, 16>) on the normalised rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import adapters, capi, synth  # noqa: E402

K = 2048
EPS = 1e-6
SENT = 0x5A5A           # bf16 bit pattern the hooks' outputs start from where a kernel must not write


def _count():
    return int(capi.lib().mtts_debug_fold_norm_launches())


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _unpack(packed, N):
    """X-fragment layout of one 32-row tile (csrc/common.h: xpack_off) -> row-major [32][N], on the host."""
    r, k = np.meshgrid(np.arange(32), np.arange(N), indexing="ij")
    off = (((k >> 4) * 64) + r + 32 * ((k >> 3) & 1)) * 8 + (k & 7)
    return packed.reshape(-1)[off]


@pytest.fixture(scope="module")
def case():
    """Inputs for 32 rows (a test with R rows takes the first R) and the expected values of every (N, R), made once."""
    g = torch.Generator(device="cuda")
    g.manual_seed(2048)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    attn, x = 0.02 * rn(32, K), 0.02 * rn(32, 2048)
    attn[1], x[1] = 0.0, 0.0                                   # residual and attention output all zero: inv = 1 / sqrt(eps)
    big = torch.rand(32, 2048, device="cuda", generator=g) < 0.5
    x[2] = torch.where(big[2], 1.0e3 * rn(2048), 1.0e-3 * rn(2048))        # both roundings of the residual add matter
    attn[2] = torch.where(big[3, :K], 30.0 * rn(K), 1.0e-3 * rn(K))
    x[0, ::2] *= 1.0e3                                         # (R = 1 has only this row)
    x[0, 1::2] *= 1.0e-2
    seq = np.arange(32, dtype=np.int32)
    seq[3] = -1                                                # an idle row between live rows
    c = dict(attn=attn.to(torch.bfloat16).contiguous(), x=x.to(torch.bfloat16).contiguous(), seq=seq,
             wo=(0.02 * rn(2048, K)).to(torch.bfloat16).contiguous(),
             norm_w=(1.0 + 0.1 * rn(2048)).to(torch.bfloat16).contiguous(),
             wgu=(0.02 * rn(288, 2048)).to(torch.bfloat16).contiguous(), expect={})
    return c


def _expect(case, monkeypatch, N, R):
    """(x' [R][N], xn [R][N]) from today's launches; cached per (N, R)."""
    if (N, R) in case["expect"]:
        return case["expect"][N, R]
    lib = capi.lib()
    monkeypatch.setenv("MTTS_GEMM_DEPTH", "1")
    wo, attn = case["wo"][:N].contiguous(), case["attn"][:R].contiguous()
    y = torch.zeros(R, N, dtype=torch.bfloat16, device="cuda")
    capi.check(lib.mtts_k_gemm_bf16(wo.data_ptr(), attn.data_ptr(), y.data_ptr(), R, N, K, 4, None))
    slab = y.float().contiguous()
    x = case["x"][:R, :N].clone()
    xn = torch.zeros(R, N, dtype=torch.bfloat16, device="cuda")
    hlast = torch.zeros(32, N, dtype=torch.bfloat16, device="cuda")
    seq, last = case["seq"][:R].copy(), np.zeros(R, dtype=np.int32)
    capi.check(lib.mtts_k_resid_norm(slab.data_ptr(), 1, N, x.data_ptr(), case["norm_w"][:N].contiguous().data_ptr(), seq.ctypes.data,
                                     last.ctypes.data, R, N, 32, EPS, xn.data_ptr(), hlast.data_ptr(), None))
    torch.cuda.synchronize()
    case["expect"][N, R] = (x, xn)
    return x, xn


@pytest.mark.parametrize("R", [32, 5, 1])
@pytest.mark.parametrize("N", [64, 2048])
def test_producer_bitwise(case, monkeypatch, N, R):
    """x' row-major and its packed copy against resid_norm_kernel's x; rows >= R of both buffers are not written."""
    lib = capi.lib()
    want, _ = _expect(case, monkeypatch, N, R)
    x = torch.full((32, N), 0, dtype=torch.int16, device="cuda")
    x[:] = SENT
    x = x.view(torch.bfloat16)
    x[:R] = case["x"][:R, :N]
    xp = torch.full((32 * N,), SENT, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    c0 = _count()
    capi.check(lib.mtts_k_oproj_resid(case["wo"][:N].contiguous().data_ptr(), case["attn"][:R].contiguous().data_ptr(), x.data_ptr(),
                                      xp.data_ptr(), R, N, None))
    torch.cuda.synchronize()
    assert _count() - c0 == 1
    got, packed = _bits(x), _unpack(_bits(xp), N)
    assert np.array_equal(got[:R], _bits(want))
    assert np.array_equal(packed[:R], _bits(want))
    assert (got[R:] == SENT).all() and (packed[R:] == SENT).all()
    assert np.count_nonzero(got[:R] != _bits(case["x"][:R, :N])) > 0.5 * (R - 1) * N     # the GEMM moved the rows (row 1 is all zero)


@pytest.mark.parametrize("R", [32, 5, 1])
@pytest.mark.parametrize("I", [48, 144])
def test_pair_bitwise(case, monkeypatch, I, R):
    """The SwiGLU output of the pair against o_proj + resid_norm + gate/up: 2 I = 96 is one pair of 48-column blocks, 288 three."""
    lib = capi.lib()
    xw, xn = _expect(case, monkeypatch, 2048, R)
    wgu = case["wgu"][:2 * I].contiguous()
    want = torch.zeros(R, I, dtype=torch.bfloat16, device="cuda")
    monkeypatch.setenv("MTTS_GEMM_DEPTH", "1")
    capi.check(lib.mtts_k_gemm_swiglu_bf16(wgu.data_ptr(), xn.data_ptr(), want.data_ptr(), R, 2 * I, 2048, None))
    x = case["x"][:R].clone()
    got = torch.zeros(R, I, dtype=torch.bfloat16, device="cuda")
    c0 = _count()
    capi.check(lib.mtts_k_fold_pair(case["wo"].data_ptr(), case["attn"][:R].contiguous().data_ptr(), x.data_ptr(), case["norm_w"].data_ptr(),
                                    wgu.data_ptr(), EPS, R, 2 * I, got.data_ptr(), None))
    torch.cuda.synchronize()
    assert _count() - c0 == 2
    assert np.array_equal(_bits(x), _bits(xw))
    assert np.array_equal(_bits(got), _bits(want))
    live = [r for r in range(R) if r != 1]
    assert np.count_nonzero(_bits(got)[live]) > 0.9 * len(live) * I
    if R > 1:
        assert not _bits(got)[1].any()                         # silu(0) * 0 of the all-zero row


def test_pair_hook_argument_errors(case):
    lib = capi.lib()
    y = torch.zeros(32, 144, dtype=torch.bfloat16, device="cuda")
    x = case["x"].clone()
    call = lambda R, N: lib.mtts_k_fold_pair(case["wo"].data_ptr(), case["attn"].data_ptr(), x.data_ptr(), case["norm_w"].data_ptr(),
                                             case["wgu"].data_ptr(), EPS, R, N, y.data_ptr(), None)
    assert call(0, 96) == capi.EINVAL and call(33, 96) == capi.EINVAL and call(5, 64) == capi.EINVAL and call(5, 128) == capi.EINVAL


# ---- engines ------------------------------------------------------------------------------------------------------------
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


def _adapter(cfg, seed, rank=4):
    rng = np.random.default_rng(seed)
    out = {}
    for n in range(cfg["num_hidden_layers"]):
        for p in adapters.PROJECTIONS:
            o, i = adapters.projection_shape(cfg, p)
            out[f"model.language_model.layers.{n}.{p}.weight"] = ((rng.standard_normal((rank, i)) * 0.05).astype(np.float32),
                                                                  (rng.standard_normal((o, rank)) * 0.05).astype(np.float32))
    return out


def _run(monkeypatch, cfg, env, batches, plen, steps, max_seq_len, adapter_row=None):
    """One engine under `env`; per batch size a ragged prompt and `steps` sampled steps -> (ids, logits bits), launches counted."""
    from mtts.engine import Engine
    for k in ("MTTS_FOLD_NORM", "MTTS_GEMM_DEPTH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MTTS_GRAPHS", "1")
    c0 = _count()
    eng = Engine(cfg, max_batch=max(batches), max_seq_len=max_seq_len)
    for name, t in _rand_weights(cfg, 5):
        eng.bind(name, t)
    if adapter_row is not None:
        eng.load_bank_adapter(0, _adapter(cfg, 9), 1.5)
    layers = [dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.05)] * 8
    res = []
    for B in batches:
        ids, mask = synth.synth_prompts(cfg, 300 + B, B, plen, 0.4, True)
        ra = None if adapter_row is None else [0 if b == adapter_row else -1 for b in range(B)]
        eng.begin(ids, mask, ids.shape[1] + steps + 8, layers=layers, do_samples=[True] * 8, seed=13, row_adapters=ra)
        eng.step(steps)
        eng.sync_state()
        gen = eng.read_generated(steps + 8)
        l0, l17 = eng.read_logits()
        res.append((gen, l0.view(np.uint32), l17.view(np.uint32)))
    eng.close()
    return res, _count() - c0


def _same(a, b, steps):
    for (ga, l0a, l17a), (gb, l0b, l17b) in zip(a, b):
        assert ga.shape == gb.shape and ga.shape[0] >= steps
        assert np.array_equal(ga, gb)
        assert np.array_equal(l0a, l0b) and np.array_equal(l17a, l17b)


def _bench_width(layers=2):
    cfg = synth.assumed_1p7b()
    cfg["num_hidden_layers"] = layers
    return cfg


def test_engine_bitwise_at_bench_width(monkeypatch):
    """Hidden 2048 / intermediate 6144 / 16 + 8 heads, two layers: batch 32 and batch 7, ragged prompts of up to 300 tokens,
    24 sampled steps under graph replay.  Ids and the last step's logits with the switch on against off; the new kernels
    run in the first leg (two per layer and batch size, counted at capture) and not in the second."""
    cfg, steps = _bench_width(), 24
    on, n_on = _run(monkeypatch, cfg, {"MTTS_FOLD_NORM": "1"}, (32, 7), 300, steps, 448)
    off, n_off = _run(monkeypatch, cfg, {"MTTS_FOLD_NORM": "0"}, (32, 7), 300, steps, 448)
    assert n_on >= 2 * 2 * 2 and n_off == 0
    _same(on, off, steps)


FALLBACKS = {
    "tiny_dims": (None, {}, (32, 5), None),                    # hidden 256: neither GEMM has the specialised shape
    "small_path": (2, {}, (3,), None),                         # B <= 4 dialogues: forward_small
    "adapter_row": (2, {}, (6,), 2),                           # a pass with an adapter row sums one slab more
    "depth_off": (2, {"MTTS_GEMM_DEPTH": "0"}, (7,), None),    # the depth-specialised kernels are switched off
}


@pytest.mark.parametrize("which", sorted(FALLBACKS))
def test_fallbacks_issue_todays_launches(monkeypatch, which):
    """With the switch on, a step that does not qualify runs no new kernel and gives what the switch off gives."""
    layers, env, batches, adapter_row = FALLBACKS[which]
    cfg = synth.tiny() if layers is None else _bench_width(layers)
    steps = 12
    on, n_on = _run(monkeypatch, cfg, dict(env, MTTS_FOLD_NORM="1"), batches, 150, steps, 320, adapter_row)
    off, n_off = _run(monkeypatch, cfg, dict(env, MTTS_FOLD_NORM="0"), batches, 150, steps, 320, adapter_row)
    assert n_on == 0 and n_off == 0
    _same(on, off, steps)
