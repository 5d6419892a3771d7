"""Sealed weight streams (csrc/gemm_sealed.hip; include/mtts.h: mtts_k_wseal, mtts_k_gemm_sealed).  -m gpu.

gate/up, down_proj and the heads exist a second time in the sealed 13-bit form of the KV pages and the one-row-tile decode
GEMMs read that.  The form is lossless and the sealed kernels keep every sum tree of the bf16 kernels, so everything here is
compared as BITS: the sealer against the format's oracle, each sealed kernel against launch_gemm on the same packed array,
the engine with MTTS_W_SEAL=2 against 0.  mtts_debug_wseal_launches shows which kernels ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import wseal_ref as wr  # noqa: E402
from mtts import capi, synth  # noqa: E402

UNSEALED_CAP = 0.10             # tests/test_wseal_cpu.py: test_the_gpu_tests_weights_seal
EPI_PARTIAL, EPI_BF16, EPI_SILU = 0, 1, 2
NINE = np.array([(0x3f - j) << 8 for j in range(9)], dtype=np.uint16)        # 9 distinct high bytes: 9 binade pairs


def _launches():
    return int(capi.lib().mtts_debug_wseal_launches())


# ---- the sealer against the oracle ------------------------------------------------------------------------------------
def _sealer_case(ktw, seed):
    rng = np.random.default_rng(seed)
    N, K = 64, 2 * 16 * ktw                                       # 2 tiles x 2 groups
    bits = wr.bf16_bits(0.02 * rng.standard_normal((N, K), dtype=np.float32))
    bits[3, 0:K // 2:16][:9] = NINE                               # tile 0, group 0, lane 3: does not fit
    bits[40, K // 2 + 8::16][:9] = NINE                           # tile 1, group 1, lane 32 + 8
    bits[5, :64] = rng.integers(0, 0x80, 64)                      # denormals
    bits[6, :64] = np.where(rng.random(64) < 0.5, 0x7f80, 0xffc1)
    bits[7, :64] = np.where(rng.random(64) < 0.5, 0x0000, 0x8000)
    bits[33] = rng.integers(0, 1 << 16, K)                        # random bits
    return bits


@pytest.mark.parametrize("ktw", [16, 12])
def test_sealer_matches_the_oracle_byte_for_byte(ktw):
    bits = _sealer_case(ktw, 3 + ktw)
    N, K = bits.shape
    groups = wr.groups_of(bits, ktw)                              # [2][2][64][8 ktw]
    packed = torch.from_numpy(wr.packed_of(groups).view(np.int16)).cuda()
    nu = ktw // 2 + ktw // 4 + 1
    out = torch.zeros(N // 32, K // (16 * ktw), nu, 64, 16, dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().mtts_k_wseal(packed.data_ptr(), N // 32, K, ktw, out.data_ptr(), None))
    got = out.cpu().numpy()
    unfit = 0
    for nt in range(N // 32):
        for c in range(K // (16 * ktw)):
            want, fit = wr.seal_group(groups[nt, c])
            assert np.array_equal(got[nt, c], want), (nt, c)
            unfit += int((~fit).sum())
    assert unfit >= 3                                             # the two built lanes and the random-bits row
    assert not np.array_equal(got, np.zeros_like(got))


# ---- kernel against kernel ------------------------------------------------------------------------------------------
# (kind, N, K, epi, split-K, k-tiles per wave): the smallest shapes the specialised kernels accept (K is the template's)
SHAPES = [("gate_up", 96, 2048, EPI_SILU, 1, 16), ("gate_up", 192, 2048, EPI_SILU, 1, 16),
          ("down", 32, 6144, EPI_PARTIAL, 4, 12), ("down", 64, 6144, EPI_PARTIAL, 4, 12),
          ("head", 70, 2048, EPI_BF16, 1, 16), ("head", 1030, 2048, EPI_BF16, 1, 16)]
# the heads' forms: one tile per block, the persistent kernel on one block per CU, and on 2 / 4 blocks (N = 70: 2 + 1 tiles;
# N = 1030: 9 + 8 + 8 + 8 tiles -- a block's tile loop, leaving it after an odd and after an even number of tiles)
HEAD_FORMS = {70: (0, 1, 2), 1030: (0, 1, 4)}


def _weights(kind, N, K, ktw, variant, seed):
    """-> (bits uint16 [N][K], expected number of not-sealed groups or None)."""
    rng = np.random.default_rng(seed)
    bits = wr.bf16_bits(0.02 * rng.standard_normal((N, K), dtype=np.float32))
    span = 16 * ktw
    if variant == "gaussian":
        return bits, None
    if variant == "one_lane":                                     # lane 5 of one group holds 9 binade pairs: one wave falls back
        r, c = min(37, N - 1), (K // span) - 2
        bits[r, c * span:(c + 1) * span:16][:9] = NINE
        want = 1
        return bits, want
    if variant == "all_flagged":
        Npad = (N + 31) // 32 * 32
        for nt in range(Npad // 32):
            if nt * 32 < N:
                for c in range(K // span):
                    bits[nt * 32, c * span:(c + 1) * span:16][:9] = NINE
        return bits, None
    assert variant == "special"
    m = rng.random((N, K))
    bits[m < 0.01] = 0x0000
    bits[(m >= 0.01) & (m < 0.02)] = 0x8000
    bits[(m >= 0.02) & (m < 0.03)] = rng.integers(1, 0x80, int(((m >= 0.02) & (m < 0.03)).sum()))
    bits[2, 100] = 0x7f80
    bits[min(9, N - 1), 300] = 0xff80
    bits[min(20, N - 1), 77] = 0xffc1
    bits[min(20, N - 1), 1500] = 0x7fc0
    return bits, None


@pytest.mark.parametrize("variant", ["gaussian", "one_lane", "all_flagged", "special"])
@pytest.mark.parametrize("M", [32, 5])
@pytest.mark.parametrize("kind,N,K,epi,ksplit,ktw", SHAPES)
def test_sealed_kernel_gives_the_bf16_kernels_bits(kind, N, K, epi, ksplit, ktw, M, variant):
    lib = capi.lib()
    bits, _ = _weights(kind, N, K, ktw, variant, 100 + N + M)
    rng = np.random.default_rng(7 + N + M)
    x = rng.standard_normal((M, K), dtype=np.float32)
    x[0, ::5] = 0.0
    w = torch.from_numpy(bits.view(np.int16)).cuda()
    xt = torch.from_numpy(wr.bf16_bits(x).view(np.int16)).cuda()
    Npad = (N + 31) // 32 * 32
    n_out = {EPI_PARTIAL: ksplit * 32 * Npad * 2, EPI_BF16: 32 * Npad, EPI_SILU: 32 * Npad // 2}[epi]     # in 16-bit words
    st = np.zeros(2, dtype=np.int64)

    def run(sealed, form):
        out = torch.full((n_out,), 0x5a5a, dtype=torch.int16, device="cuda")
        c0 = _launches()
        capi.check(lib.mtts_k_gemm_sealed(w.data_ptr(), xt.data_ptr(), out.data_ptr(), M, N, K, epi, ksplit, sealed, form,
                                          st.ctypes.data, None))
        assert _launches() - c0 == (1 if sealed else 0)
        return out.cpu().numpy().view(np.uint16)

    ref = run(0, 0)
    groups = (Npad // 32) * (K // (16 * ktw))
    assert st[0] == groups
    want_bad = wr.unsealed_share(np.concatenate([bits, np.zeros((Npad - N, K), np.uint16)]), ktw) * groups
    assert st[1] == round(want_bad)
    if variant == "one_lane":
        assert st[1] == 1
    if variant == "all_flagged":
        assert st[1] == groups
    if variant == "gaussian":
        assert st[1] <= UNSEALED_CAP * groups
    for form in (HEAD_FORMS[N] if kind == "head" else (0,)):
        got = run(1, form)
        assert np.array_equal(got, ref), (kind, N, M, variant, form)
    # it is a product, and nothing outside the output was written: the padding columns of a head keep the hook's sentinel
    assert len(np.unique(ref)) > 16
    if epi == EPI_BF16 and Npad > N:
        assert (ref.reshape(32, Npad)[:, N:] == 0xa5a5).all()
    if variant == "special":
        f = (ref.astype(np.uint32) << 16).view(np.float32) if epi != EPI_PARTIAL else ref.view(np.float32)
        assert np.isnan(f).any()                                   # NaNs are there and were compared as bits


# ---- the engine -----------------------------------------------------------------------------------------------------
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


def _adapter(cfg, seed):
    """LoRA pairs on gate / up / down of both layers: name -> (A [r, in], B [out, r])."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    H, I, r = cfg["hidden_size"], cfg["intermediate_size"], 8
    out = {}
    for n in range(cfg["num_hidden_layers"]):
        for proj, (o, i) in (("gate_proj", (I, H)), ("up_proj", (I, H)), ("down_proj", (H, I))):
            out["model.language_model.layers.%d.mlp.%s.weight" % (n, proj)] = (
                0.05 * torch.randn(r, i, device="cuda", generator=g), 0.05 * torch.randn(o, r, device="cuda", generator=g))
    return out


def _engine_run(monkeypatch, mode, cfg, steps):
    from mtts.engine import Engine
    monkeypatch.setenv("MTTS_W_SEAL", mode)
    monkeypatch.setenv("MTTS_GRAPHS", "1")
    eng = Engine(cfg, max_batch=32, max_seq_len=256)
    weights = dict(_rand_weights(cfg, 5))
    for name, t in weights.items():
        eng.bind(name, t)
    adapter = _adapter(cfg, 9)
    layers = [dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.05)] * 8
    res, stats = [], []
    for phase in ("base", "adapter merged", "adapter unloaded"):
        if phase != "base":
            eng.sched_open(32, 64)                                # ends the run: weights cannot change while one is open
        if phase == "adapter merged":                            # what load_adapter does: merge-and-pack binds
            for name, (A, B) in adapter.items():
                eng.bind_lora(name, weights[name], A, B, 0.5)
        if phase == "adapter unloaded":                           # what unload_adapter does: the base matrices again
            for name in adapter:
                eng.bind(name, weights[name])
        for B in (32, 3):
            ids, mask = synth.synth_prompts(cfg, 300 + B, B, 40, 0.4, True)
            eng.begin(ids, mask, ids.shape[1] + steps + 8, layers=layers, do_samples=[True] * 8, seed=13)
            eng.step(steps)
            eng.sync_state()
            gen = eng.read_generated(steps + 8)
            l0, l17 = eng.read_logits()
            res.append((gen, l0.view(np.uint32), l17.view(np.uint32)))
        if mode != "0":
            stats.append(eng.wseal_stats())
    assert eng.close() == 0
    return res, stats


def test_engine_bitwise_at_bench_width_and_across_rebinds(monkeypatch):
    """Hidden 2048 / intermediate 6144 / the full vocabularies, two layers: batch 32 (the sealed kernels) and batch 3 (the
    small-batch path, which keeps the bf16 arrays), 20 sampled steps under graph replay, before an adapter, with one merged
    into gate / up / down (every such bind re-seals) and after the base matrices came back."""
    cfg = synth.assumed_1p7b()
    cfg["num_hidden_layers"] = 2
    steps = 20
    c0 = _launches()
    on, stats = _engine_run(monkeypatch, "2", cfg, steps)
    c1 = _launches()
    off, _ = _engine_run(monkeypatch, "0", cfg, steps)
    assert _launches() == c1                                      # MTTS_W_SEAL=0: no sealed launch
    # gate/up and down_proj of two layers and the two head GEMMs, captured at least once in each of the three phases
    assert c1 - c0 >= 3 * (2 * 2 + 2)
    for (ga, l0a, l17a), (gb, l0b, l17b) in zip(on, off):
        assert ga.shape == gb.shape and ga.shape[0] >= steps
        assert np.array_equal(ga, gb)
        assert np.array_equal(l0a, l0b) and np.array_equal(l17a, l17b)
    # the merged adapter changed the run (the re-sealed twins were read, not stale ones), its removal brought it back
    assert not np.array_equal(on[0][1], on[2][1])
    assert np.array_equal(on[0][0], on[4][0]) and np.array_equal(on[0][1], on[4][1])
    for st in stats:
        for kind, s in st.items():
            print(kind, s)
            assert s["groups"] > 0 and s["on"]
            assert s["unsealed"] <= UNSEALED_CAP * s["groups"], kind
    H, I, V0p, Vsp = 2048, 6144, (cfg["vocab_size"] + 31) // 32 * 32, (cfg["speech_vocab_size"] + 31) // 32 * 32
    assert stats[0]["gate_up"]["groups"] == 2 * (2 * I // 32) * 8 and stats[0]["down"]["groups"] == 2 * (H // 32) * 32
    assert stats[0]["head0"]["groups"] == V0p // 32 * 8 and stats[0]["heads17"]["groups"] == 7 * Vsp // 32 * 8


def test_default_policy_reads_down_proj_and_the_heads_sealed(monkeypatch):
    """MTTS_W_SEAL=1 (the default): gate/up keeps no twin (it did not win its launch trains), down_proj and the heads read
    theirs at the share of not-sealed groups Gaussian weights have."""
    from mtts.engine import Engine
    monkeypatch.delenv("MTTS_W_SEAL", raising=False)
    monkeypatch.setenv("MTTS_GRAPHS", "1")
    cfg = synth.assumed_1p7b()
    cfg["num_hidden_layers"] = 1
    eng = Engine(cfg, max_batch=32, max_seq_len=128)
    for name, t in _rand_weights(cfg, 5):
        eng.bind(name, t)
    st = eng.wseal_stats()
    assert st["gate_up"] == dict(groups=0, unsealed=0, on=False)
    for kind, bound in (("down", 512), ("head0", 8), ("heads17", 64)):          # engine.h: WSEAL_MAX_UNSEALED
        assert st[kind]["on"] and st[kind]["unsealed"] <= st[kind]["groups"] / bound, (kind, st[kind])
    ids, mask = synth.synth_prompts(cfg, 300, 32, 40, 0.4, True)
    c0 = _launches()
    eng.begin(ids, mask, ids.shape[1] + 16)
    eng.step(4)
    eng.sync_state()
    assert _launches() - c0 >= 3                                  # down_proj and the two head GEMMs (graphs: counted at capture)
    assert eng.close() == 0
