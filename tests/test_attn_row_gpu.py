"""Whole-row decode attention (csrc/attn.hip: attn_row_kernel, one launch per layer, one block per (row, kv head))
against the launches it replaces: attn_scores + attn_pv + attn_combine.  -m gpu.

The row kernel keeps every rounding point and every summation order of the two-pass kernels, so everything here is
compared BITWISE: the X-fragment output rows, the bf16 K / V pools after the launch (the new rows included) and the
sealed pools, through mtts_k_attn_section (one layer's attention section on given qkv slabs, either path); then whole
engines, MTTS_ATTN_ROW=2 (whenever the LDS fits) and auto against 0.  mtts_debug_attn_row_launches counts the row
kernel's launches, so the comparisons also check which leg ran it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402

NKV = 2
EPS = 1e-6
# context lengths WITH the new token: 1 = first token of the first page; 63, 64, 65 = a page completing; 129 = an odd
# number of pages (a one-page work item); 512, 513 = a chunk boundary; 1089 = 18 pages = 3 chunks, the last one partial,
# more work items than waves
LENGTHS = (1, 63, 64, 65, 129, 512, 513, 1089)
RAGGED = (1089, 0, 65, 300, 513)          # 5 rows, one idle
LONG = (4161, 4097)                       # 66 and 65 pages: statistics pairs beyond the first 64 (the bench's own context)


def _bf(t):
    return t.to(torch.bfloat16).contiguous()


def _inputs(lens, nq, ksplit, seed, wild=True):
    """Slabs, norm weights, RoPE tables and the cached K / V of `lens` rows; `wild`: the longest row gets pages that do
    not seal (K and V), K dims on different scales and V tokens too quiet for their page's scale."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    R, Lmax = len(lens), (max(lens) + 63) // 64 * 64
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    slabs = (rn(ksplit, R, (nq + 2 * NKV) * 128) * (2.0 / ksplit ** 0.5)).contiguous()
    qnw, knw = _bf(1.0 + 0.1 * rn(128)), _bf(1.0 + 0.1 * rn(128))
    pos = torch.arange(Lmax, device="cuda", dtype=torch.float32)[:, None]
    ang = pos * (1.0e6 ** (-torch.arange(64, device="cuda", dtype=torch.float32) / 64.0))[None, :]
    cos, sin = _bf(torch.cos(ang)), _bf(torch.sin(ang))
    K, V = rn(R, Lmax, NKV, 128), rn(R, Lmax, NKV, 128)
    e = lambda lo, hi, *s: 2.0 ** torch.randint(lo, hi, s, device="cuda", generator=g).float()
    big = int(np.argmax(lens))
    if wild and lens[big] > 640:
        K[big, 100:140] *= e(-40, 1, 40, NKV, 128)              # tokens whose K row cannot seal: the in-kernel bf16 fallback
        V[big, 200:300, :, 8:12] *= e(-40, 1, 100, NKV, 4)      # a V lane that cannot
        K[big, 320:640] *= e(-3, 4, 1, NKV, 128)                # dims on different scales: seals, q is rescaled
    if wild and lens[big] > 720:
        V[big, 700:720] *= 2.0 ** -110                          # tokens so quiet that a probability's rescale leaves the normal range
    return slabs, qnw, knw, cos, sin, _bf(K), _bf(V), R, Lmax


def _section(inp, lens, nq, ksplit, sealed, path, table):
    slabs, qnw, knw, cos, sin, K, V, R, Lmax = inp
    pages = R * (Lmax // 64)
    out = torch.zeros(32, nq * 128, dtype=torch.bfloat16, device="cuda")
    kc = torch.zeros(NKV, pages, 64 * 128, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    kp = torch.zeros(NKV, pages, 13 * 64 * 16, dtype=torch.uint8, device="cuda")
    vp = torch.zeros_like(kp)
    hl = np.asarray(lens, dtype=np.int32)
    capi.check(capi.lib().mtts_k_attn_section(
        slabs.data_ptr(), ksplit, qnw.data_ptr(), knw.data_ptr(), cos.data_ptr(), sin.data_ptr(), EPS, K.data_ptr(), V.data_ptr(),
        hl.ctypes.data, table.ctypes.data, R, Lmax, nq, NKV, sealed, path, out.data_ptr(), kc.data_ptr(), vc.data_ptr(),
        kp.data_ptr(), vp.data_ptr(), None))
    torch.cuda.synchronize()
    return [t.view(torch.int16).cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy() for t in (out, kc, vc, kp, vp)]


def _count():
    return int(capi.lib().mtts_debug_attn_row_launches())


def _compare(lens, G, sealed, ksplit, seed, wild=True):
    nq = G * NKV
    inp = _inputs(lens, nq, ksplit, seed, wild)
    R, Lmax = inp[-2], inp[-1]
    table = np.random.default_rng(seed).permutation(R * (Lmax // 64)).astype(np.int32).reshape(R, Lmax // 64)
    c0 = _count()
    two = _section(inp, lens, nq, ksplit, sealed, 0, table)
    assert _count() == c0
    row = _section(inp, lens, nq, ksplit, sealed, 1, table)
    assert _count() == c0 + 1
    for name, a, b in zip(("output rows", "K pool", "V pool", "sealed K pool", "sealed V pool"), two, row):
        assert np.array_equal(a, b), name
    return inp, table, row


@pytest.mark.parametrize("ksplit", [1, 4])
@pytest.mark.parametrize("sealed", [0, 1])
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("lens", [LENGTHS, RAGGED], ids=["lengths", "ragged-idle"])
def test_row_path_equals_two_pass_bitwise(lens, G, sealed, ksplit):
    inp, table, (out, kc, vc, kp, vp) = _compare(lens, G, sealed, ksplit, 40 + 7 * G + ksplit)
    nq = G * NKV
    # output [32][nq*128] in the X-fragment layout [k/16][half][row][8] -> row-major
    o = out.reshape(nq * 8, 2, 32, 8).transpose(2, 0, 1, 3).reshape(32, nq * 128)
    for r, n in enumerate(lens):
        assert (np.count_nonzero(o[r]) > 0) == (n > 0)       # live rows attend, the idle row is written as zeros
    assert np.count_nonzero(o[len(lens):]) == 0
    # the new K and V rows reached the pools: token n - 1 of page table[r][(n - 1) / 64]
    for r, n in enumerate(lens):
        if n:
            pg, t = table[r][(n - 1) // 64], (n - 1) % 64
            assert np.count_nonzero(kc[:, pg].reshape(NKV, 16, 64, 8)[:, :, t]) > 100
            assert np.count_nonzero(vc[:, pg].reshape(NKV, 32, 128, 2)[:, t // 2, :, t % 2]) > 100


def test_row_path_beyond_64_pages_bitwise():
    """65 and 66 pages: the row-wide statistics take the strided pairs beyond lane 63's, 9 chunks, 33 work items."""
    _compare(LONG, 2, 1, 4, 91)


def test_section_is_the_reference_attention():
    """The hook's output is attention: fp32 restatement (slab sum -> bf16, per-head RMSNorm, RoPE, softmax(q.k / sqrt(d)) v)
    of the `lengths` launch at G = 2.  Not a precision test of the kernels (tests/test_scores_gpu.py and the oracle tests
    are): it guards the bitwise comparisons above against two paths that agree on nothing.  Tolerance: the kernels round
    the scores to bf16 twice (|s| <= 16 here: 16 * 2^-8 in the exponent, 6 % of a probability) and the probabilities once."""
    G, ksplit, lens = 2, 4, LENGTHS
    nq = G * NKV
    inp, table, (out, kc, vc, kp, vp) = _compare(lens, G, 1, ksplit, 17, wild=False)
    slabs, qnw, knw, cos, sin, K, V, R, Lmax = inp
    r16 = lambda t: t.to(torch.bfloat16).float()
    x = r16(slabs.sum(0)).reshape(R, nq + 2 * NKV, 128)

    def norm_rope(h, w, n):
        h = r16(w.float() * r16(h * torch.rsqrt((h * h).mean(-1, keepdim=True) + EPS)))
        c, s = cos[n - 1].float(), sin[n - 1].float()
        a, b = h[..., :64], h[..., 64:]
        return torch.cat([r16(r16(a * c) + r16(-b * s)), r16(r16(b * c) + r16(a * s))], -1)

    o = torch.from_numpy(out.reshape(nq * 8, 2, 32, 8).transpose(2, 0, 1, 3).reshape(32, nq * 128).copy()).cuda().view(torch.bfloat16).float()
    for r, n in enumerate(lens):
        q = norm_rope(x[r, :nq], qnw, n)
        k = torch.cat([K[r, :n - 1].float(), norm_rope(x[r, nq:nq + NKV], knw, n)[None]], 0)       # [n][nkv][128]
        v = torch.cat([V[r, :n - 1].float(), x[r, nq + NKV:][None]], 0)
        for h in range(nq):
            s = (k[:, h // G] @ q[h]) / 128.0 ** 0.5
            assert float(s.abs().max()) <= 16.0
            ref = torch.softmax(s, 0) @ v[:, h // G]
            got = o[r, h * 128:(h + 1) * 128]
            assert float((got - ref).abs().max()) <= 0.07 * float(ref.abs().max()) + 1e-3, (r, h)


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


def _run(monkeypatch, cfg, row, graphs, lens, steps, max_seq_len):
    """One engine: prompts of exactly `lens` tokens, `steps` sampled steps -> (generated ids, last-step logits bits)."""
    from mtts.engine import Engine
    monkeypatch.setenv("MTTS_ATTN_ROW", row)
    monkeypatch.setenv("MTTS_GRAPHS", graphs)
    eng = Engine(cfg, max_batch=len(lens), max_seq_len=max_seq_len)
    for name, t in _rand_weights(cfg, 5):
        eng.bind(name, t)
    seqs = [synth.synth_prompts(cfg, 300 + i, 1, n, 0.4, False)[0][0] for i, n in enumerate(lens)]
    ids, mask = synth.left_pad(seqs, cfg["pad_token_id"])
    layers = [dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.05)] * 8
    eng.begin(ids, mask, ids.shape[1] + steps + 8, layers=layers, do_samples=[True] * 8, seed=13)
    eng.step(steps)
    eng.sync_state()
    gen = eng.read_generated(steps + 8)
    l0, l17 = eng.read_logits()
    res = (gen, l0.view(np.uint32).copy(), l17.view(np.uint32).copy())
    eng.close()
    return res


def _same(a, b, steps):
    assert a[0].shape == b[0].shape and a[0].shape[0] >= steps
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("graphs", ["1", "0"])
def test_tiny_engine_row_against_two_pass(monkeypatch, graphs):
    """Tiny dims, 5 dialogues (above the small-batch path), the long prompts end at position 60: 12 sampled steps cross the
    page boundary at 64.  MTTS_ATTN_ROW=2 against 0: same tokens, same last-step logits; captured steps and plain launches."""
    cfg = synth.tiny()
    lens, steps = (61, 61, 35, 61, 50), 12
    c0 = _count()
    on = _run(monkeypatch, cfg, "2", graphs, lens, steps, 256)
    c1 = _count()
    off = _run(monkeypatch, cfg, "0", graphs, lens, steps, 256)
    assert c1 - c0 >= cfg["num_hidden_layers"] and _count() == c1
    _same(on, off, steps)


def test_bench_width_engine_takes_the_row_kernel_by_itself(monkeypatch):
    """Hidden 2048, 16 / 8 heads, 2 layers, 32 dialogues of 300 tokens, 4 steps under auto (MTTS_ATTN_ROW=1): rows x kv
    heads = 256 fills the machine, the row kernel runs (counter), and the tokens are those of MTTS_ATTN_ROW=0."""
    cfg = synth.assumed_1p7b()
    cfg["num_hidden_layers"] = 2
    lens, steps = (300,) * 32, 4
    c0 = _count()
    auto = _run(monkeypatch, cfg, "1", "1", lens, steps, 512)
    c1 = _count()
    off = _run(monkeypatch, cfg, "0", "1", lens, steps, 512)
    assert c1 - c0 >= 2 and _count() == c1
    _same(auto, off, steps)
