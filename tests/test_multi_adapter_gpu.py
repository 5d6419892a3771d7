"""Per-dialogue LoRA adapters in one batch (csrc/multilora.hip; mtts_adapter_load, mtts_set_row_adapters,
generate(adapter_names=...)).  -m gpu.

The delta of a row's adapter is defined down to the order of its operations (mtts/adapters.py: delta_spec), so the kernel
has one right answer per element, and it is a function of the row alone: every engine comparison here is bitwise -- a row
without an adapter against an engine with an empty bank, a row with one against its batch-1 run."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import adapters, capi, synth  # noqa: E402

PFCAP = 2048                     # csrc/common.h: MTTS_PFCAP, the row stride of the split-K slabs
SENTINEL = np.uint32(0x7FC0ABCD)
SAMPLED = ([dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.2)] * 8, [True] * 8)
GREEDY = (None, None)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. lora_delta_kernel against delta_spec ------------------------------------------------------------------------------------
# name: (Npad, [(col0, ncols, mul) of each matrix of the slab], matrices each of the two adapters targets)
PLACEMENTS = {
    "padded_80_of_96": (96, [(0, 80, 1)], [(0,), (0,)]),                                   # o / down: padding columns 80..95
    "k_in_qkv": (256, [(0, 128, 1), (128, 64, 1), (192, 64, 1)], [(0, 1, 2), (1,)]),       # adapter 1 targets k alone
    "gate_up_interleaved": (96, [(0, 48, 2), (1, 48, 2)], [(0, 1), (1,)]),
}
# the shapes of the 1.7B model's launches: several blocks of 1024 columns per row (matrices that start and end inside a
# block's columns or span several blocks), and rows long enough that a lane's partial sum takes more than one term group
LARGE = {
    "qkv_4096": (4096, [(0, 2048, 1), (2048, 1024, 1), (3072, 1024, 1)], [(0, 1, 2), (1,)]),
    "qkv_uneven_2560": (2560, [(0, 1500, 1), (1500, 548, 1), (2048, 500, 1)], [(0, 2), (0, 1, 2)]),    # boundaries inside blocks, 12 padding columns
    "gate_up_4096": (4096, [(0, 2048, 2), (1, 2048, 2)], [(0, 1), (1,)]),
    "down_padded_2016_of_2048": (2048, [(0, 2016, 1)], [(0,), (0,)]),
}


@pytest.mark.parametrize("K", [48, 144, 256])
@pytest.mark.parametrize("place", list(PLACEMENTS))
def test_lora_delta_kernel_bitwise_vs_spec(place, K):
    _check_delta(PLACEMENTS[place], K, (1, 16, 33, 64), (1, 5, 33, 70))


@pytest.mark.parametrize("place,K", [("qkv_4096", 2048), ("qkv_uneven_2560", 2048), ("gate_up_4096", 2048), ("down_padded_2016_of_2048", 6144)])
def test_lora_delta_kernel_bitwise_vs_spec_at_model_shapes(place, K):
    _check_delta(LARGE[place], K, (16,), (5, 33))


def _check_delta(placement, K, ranks, row_counts):
    Npad, segs, targets = placement
    lib = capi.lib()
    nseg = len(segs)
    hseg = np.ascontiguousarray(segs, dtype=np.int32)
    for r in ranks:
        rng = np.random.default_rng(1000 * K + r)
        mats, keep = {}, []
        pa, pb = (C.c_void_p * (2 * nseg))(), (C.c_void_p * (2 * nseg))()
        hr, hs = np.zeros(2 * nseg, np.int32), np.zeros(2 * nseg, np.float32)
        for a in range(2):
            for s in targets[a]:
                A = (rng.standard_normal((r, K)) * 0.1).astype(np.float32)
                B = (rng.standard_normal((segs[s][1], r)) * 0.1).astype(np.float32)
                sc = np.float32(2.7 if a == 0 else 0.3)          # not powers of two: the scaling multiply rounds
                ta, tb = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
                keep += [ta, tb]
                mats[a, s] = (A, B, sc)
                pa[a * nseg + s], pb[a * nseg + s] = ta.data_ptr(), tb.data_ptr()
                hr[a * nseg + s], hs[a * nseg + s] = r, sc
        for R in row_counts:
            x = synth.round_bf16(rng.standard_normal((R, K)).astype(np.float32))
            row_ad = rng.integers(-2, 2, R).astype(np.int32)     # -2 idle row, -1 no adapter, 0 / 1
            row_ad[:min(R, 3)] = [0, -1, 1][:min(R, 3)]
            want = np.full((3, PFCAP, Npad), SENTINEL, dtype=np.uint32)
            want[1, :R] = 0                                      # +0.0: rows without adapter, untargeted matrices, padding
            for a in range(2):
                rows = np.nonzero(row_ad == a)[0]
                for s in targets[a]:
                    if len(rows):
                        A, B, sc = mats[a, s]
                        col0, ncols, mul = segs[s]
                        want[1, rows[:, None], col0 + mul * np.arange(ncols)[None, :]] = _bits(adapters.delta_spec(x[rows], A, B, sc))
            slabs = torch.from_numpy(np.full((3, PFCAP, Npad), SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
            xt = torch.from_numpy(x).to(torch.bfloat16).cuda()
            capi.check(lib.mtts_k_lora_delta(xt.data_ptr(), R, K, Npad, nseg, hseg.ctypes.data, 2, pa, pb, hr.ctypes.data, hs.ctypes.data,
                                             row_ad.ctypes.data, slabs.data_ptr(), 1, None))
            got = slabs.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), (r, R, "a neighbouring slab was written")
            assert np.array_equal(got[1, R:], want[1, R:]), (r, R, "rows past R were written")
            bad = np.argwhere(got[1, :R] != want[1, :R])
            assert len(bad) == 0, (r, R, len(bad), bad[:5], row_ad[bad[:5, 0]])
            assert (want[1, :R] != 0).any() or not (row_ad >= 0).any()


def test_lora_delta_hook_argument_errors():
    lib = capi.lib()
    t = torch.zeros(3 * PFCAP * 32, dtype=torch.float32, device="cuda")
    x = torch.zeros(4 * 48, dtype=torch.bfloat16, device="cuda")
    seg = np.array([[0, 32, 1]], np.int32)
    pa, pb = (C.c_void_p * 1)(t.data_ptr()), (C.c_void_p * 1)(t.data_ptr())
    sc, rows = np.ones(1, np.float32), np.zeros(4, np.int32)

    def call(R=4, K=48, Npad=32, r=4, seg=seg, rows=rows):
        hr = np.array([r], np.int32)
        return lib.mtts_k_lora_delta(x.data_ptr(), R, K, Npad, 1, seg.ctypes.data, 1, pa, pb, hr.ctypes.data, sc.ctypes.data,
                                     rows.ctypes.data, t.data_ptr(), 0, None)

    assert call() == 0
    assert call(K=40) == capi.EINVAL and call(Npad=48) == capi.EINVAL and call(r=65) == capi.EINVAL and call(R=0) == capi.EINVAL
    assert call(seg=np.array([[8, 32, 1]], np.int32)) == capi.EINVAL                 # the matrix does not fit the slab
    assert call(rows=np.array([0, 1, 0, 0], np.int32)) == capi.EINVAL                # adapter 1 of 1


# ---- 2. swiglu_slabs_kernel -------------------------------------------------------------------------------------------------------
def _rbf(a):
    return synth.round_bf16(np.asarray(a, dtype=np.float32))


@pytest.mark.parametrize("M,N,K", [(5, 192, 144), (33, 192, 256), (70, 1024, 64),
                                   (5, 4224, 64)])        # N / 2 > 2048: more than one block per row
def test_swiglu_slabs_kernel(M, N, K):
    lib = capi.lib()
    rng = np.random.default_rng(M + N)
    w = torch.from_numpy(_rbf(rng.standard_normal((N, K)) * 0.1)).to(torch.bfloat16).cuda()
    x = torch.from_numpy(_rbf(rng.standard_normal((M, K)))).to(torch.bfloat16).cuda()
    bf = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
    fused, y0, y1 = (torch.zeros(M, N // 2, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    slab0 = torch.zeros(M, N, dtype=torch.float32, device="cuda")
    capi.check(lib.mtts_k_gemm_swiglu_bf16(w.data_ptr(), x.data_ptr(), fused.data_ptr(), M, N, K, None))
    # a zero delta: the unfused form is the fused epilogue
    capi.check(lib.mtts_k_swiglu_slabs(w.data_ptr(), x.data_ptr(), None, y0.data_ptr(), slab0.data_ptr(), M, N, K, None))
    assert np.array_equal(bf(y0), bf(fused)) and np.count_nonzero(bf(y0)) > 0.5 * y0.numel()
    zero = torch.zeros(M, N, dtype=torch.float32, device="cuda")
    capi.check(lib.mtts_k_swiglu_slabs(w.data_ptr(), x.data_ptr(), zero.data_ptr(), y1.data_ptr(), None, M, N, K, None))
    assert np.array_equal(bf(y1), bf(fused))
    # a random delta: the four rounding points on slab 0 + slab 1, in numpy float32
    delta = (rng.standard_normal((M, N)) * 0.5).astype(np.float32)
    dt = torch.from_numpy(delta).cuda()
    capi.check(lib.mtts_k_swiglu_slabs(w.data_ptr(), x.data_ptr(), dt.data_ptr(), y1.data_ptr(), None, M, N, K, None))
    z = _rbf(slab0.cpu().numpy() + delta)                        # gate, up -> bf16
    g, u = z[:, 0::2], z[:, 1::2]
    a = _rbf(g / (np.float32(1) + np.exp(-g, dtype=np.float32)))         # silu(gate) -> bf16
    want = _rbf(a * u)                                           # product -> bf16
    got = y1.float().cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
    assert not np.array_equal(bf(y1), bf(fused))


# ---- engines ------------------------------------------------------------------------------------------------------------------------
from multi_adapter_case import (CFG, NL, PARITY_GATE, PARITY_STEPS, RANK, SCALING, free_decisions, merged_vs_unmerged,  # noqa: E402
                                adapter as _adapter, engine as _engine, name as _name, prompts as _prompts, weights as _weights)


def _run(eng, ids, mask, steps, mode, row_adapters=None, row_ids=None, seed=7):
    """-> (generated ids [steps, B, 8], final logits l0 [B, V0] and l17 [7, B, Vs], log-probabilities [steps, B, 8])."""
    eng.begin(ids, mask, ids.shape[1] + steps + 20, layers=mode[0], do_samples=mode[1], seed=seed, row_ids=row_ids,
              output_scores=True, row_adapters=row_adapters)
    eng.step(steps)
    s, fin = eng.sync_state()
    assert s == steps and not fin
    assert eng.seq_state()[1].all(), "a dialogue finished inside the test's steps"
    out = (eng.read_generated(steps), *eng.read_logits(), eng.read_scores(steps))
    eng.sched_open(4, 64, output_scores=True)               # ends the abandoned run
    return out


def _row(res, b):
    gen, l0, l17, lp = res
    return gen[:, b], l0[b], l17[:, b], lp[:, b]


def _same_row(x, y):
    """ids equal, logits and log-probabilities == as floats (NaN marks the same non-decisions in both)."""
    return (np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) and
            np.array_equal(np.isnan(x[3]), np.isnan(y[3])) and np.array_equal(np.nan_to_num(x[3]), np.nan_to_num(y[3])))


@pytest.fixture(scope="module")
def engines():
    bank, plain = _engine(True), _engine(False)
    yield bank, plain
    bank.close()
    plain.close()


# ---- 3. base rows are untouched -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_rows_without_adapter_equal_the_engine_with_an_empty_bank(engines, mode):
    bank, plain = engines
    ids, mask = _prompts((21, 40, 33), 5)
    base = _run(plain, ids, mask, 20, mode)
    got = _run(bank, ids, mask, 20, mode, row_adapters=[-1, 0, -1])
    assert _same_row(_row(got, 0), _row(base, 0)) and _same_row(_row(got, 2), _row(base, 2))
    assert not np.array_equal(_row(got, 1)[1], _row(base, 1)[1])            # the adapter row's logits moved
    if mode is GREEDY:
        assert not np.array_equal(_row(got, 1)[0], _row(base, 1)[0])        # ... and its greedy ids
    # lora_B all zero (PEFT's initial state): every row is the base row, also the one that carries it
    zero = _run(bank, ids, mask, 20, mode, row_adapters=[-1, 2, 2])
    assert all(_same_row(_row(zero, b), _row(base, b)) for b in range(3))
    # B = 1: the base engine takes the small-batch path, a pass with an adapter row never does
    one = _run(plain, ids[2:], mask[2:], 20, mode, row_ids=[2])
    assert _same_row(_row(one, 0), _row(base, 2))
    assert _same_row(_row(_run(bank, ids[2:], mask[2:], 20, mode, row_adapters=[2], row_ids=[2]), 0), _row(one, 0))
    # the bank engine without row adapters is the plain engine
    assert all(_same_row(_row(_run(bank, ids, mask, 20, mode), b), _row(base, b)) for b in range(3))


# ---- 4. no dependence on neighbours -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_adapter_row_equals_its_batch_1_run(engines, mode):
    """A prefill of 100 tokens (more than one page) and 72 steps: position 127 completes the second page, which is sealed
    and read in its sealed form from then on."""
    bank, _ = engines
    ids, mask = _prompts((100, 37, 64), 6)
    got = _run(bank, ids, mask, 72, mode, row_adapters=[0, 1, -1])
    for b, ad in ((0, 0), (1, 1)):
        alone = _run(bank, ids[b:b + 1], mask[b:b + 1], 72, mode, row_adapters=[ad], row_ids=[b])
        assert _same_row(_row(alone, 0), _row(got, b)), b
    other = _run(bank, ids, mask, 72, mode, row_adapters=[1, 0, -1])
    assert not np.array_equal(_row(other, 0)[1], _row(got, 0)[1])          # the two adapters are different adapters


# ---- 5. scheduler ---------------------------------------------------------------------------------------------------------------------
def _plain_prompt(rng, n):
    raw = np.full((n, 8), 1024, dtype=np.int64)
    raw[:, 0] = rng.integers(0, 151643, n)
    raw[n - 6:, 0] = 151665 + rng.integers(0, 1024, 6)
    raw[n - 6:, 1:] = rng.integers(0, 1024, (6, 7))
    return synth.shifting_inputs(raw, CFG["pad_token_id"])


def test_scheduler_keeps_each_dialogue_with_its_adapter():
    """2 slots, 5 prompts over adapters [a, b, none, a, b]: equal to the five batch-1 runs -- on a full pool, on a pool of 6
    pages that forces an eviction (the re-queued dialogue is submitted with its adapter again), and with 2 takes per
    prompt (forks inherit the source's adapter; a queued take is submitted with it)."""
    from mtts.scheduler import ContinuousBatcher
    rng = np.random.default_rng(12)
    prompts = [_plain_prompt(rng, int(rng.integers(70, 120))) for _ in range(5)]
    ads = [0, 1, -1, 0, 1]
    seeds = list(range(700, 705))
    new, n = 120, 2
    eng = _engine(True, max_batch=2, max_seq_len=384)
    try:
        want = {}
        for i, p in enumerate(prompts):
            for j in range(n):                              # take j of a prompt draws with row id j
                out = eng.generate(p[None], np.ones((1, p.shape[0])), p.shape[0] + new, layers=SAMPLED[0], do_samples=SAMPLED[1],
                                   seed=seeds[i], row_ids=[j], row_adapters=[ads[i]])
                want[i, j] = out[0]
        assert not np.array_equal(want[0, 0][-40:], eng.generate(prompts[0][None], np.ones((1, prompts[0].shape[0])), prompts[0].shape[0] + new,
                                                                  layers=SAMPLED[0], do_samples=SAMPLED[1], seed=seeds[0], row_ids=[0])[0][-40:])
        cb = ContinuousBatcher(eng, slots=2, gen_cap=new + 16, layers=SAMPLED[0], do_samples=SAMPLED[1], steps_per_poll=8)
        got = cb.run(prompts, new, seeds=seeds, adapters=ads)
        assert cb.evictions == 0
        for i in range(5):
            assert got[i].shape == want[i, 0].shape and np.array_equal(got[i], want[i, 0]), i
        cb = ContinuousBatcher(eng, slots=2, gen_cap=new + 16, layers=SAMPLED[0], do_samples=SAMPLED[1], steps_per_poll=8)
        got = cb.run(prompts, new, seeds=seeds, adapters=ads, takes=n)
        assert cb.forks > 0
        for i in range(5):
            for j in range(n):
                assert got[i * n + j].shape == want[i, j].shape and np.array_equal(got[i * n + j], want[i, j]), (i, j)
    finally:
        eng.close()
    small = _engine(True, max_batch=2, max_seq_len=384, kv_pool_pages=6)
    try:
        cb = ContinuousBatcher(small, slots=2, gen_cap=new + 16, layers=SAMPLED[0], do_samples=SAMPLED[1], steps_per_poll=8)
        got = cb.run(prompts, new, seeds=seeds, adapters=ads)
        assert cb.evictions > 0 and small.kv_pool_state()[1] == 6
        for i in range(5):
            assert got[i].shape == want[i, 0].shape and np.array_equal(got[i], want[i, 0]), i
    finally:
        small.close()


# ---- 6. against the merged path -------------------------------------------------------------------------------------------------------
def test_unmerged_row_against_the_merged_adapter():
    """The reference is this repository's merged path; the two differ by the bf16 rounding of the merged weight.

    The project's relative gate of 0.008 (PARITY_GATE, two bf16 ulps) leaves out 18 of the 356 free decisions of the 48
    greedy steps (at most a tenth may be; tests/test_multi_adapter_cpu.py checks the same for the oracle's run), but it does
    NOT hold: measured on an MI355X (tools/multi_adapter_parity.py, profiles/multi_adapter_parity.json) 8 of those 18 differ
    and ONE decision above the gate differs too -- step 9, channel 1, relative margin 0.0142, the two logits 0.0234 = three
    bf16 ulps apart.  The other misses sit one ulp (0.0078) to a few ulps apart.  The adapter of the tests is larger than the
    base weights (B A * scaling has about twice their standard deviation), so the rounding of the merged weight moves the
    logits by more than the noise the gate was set for: the largest absolute logit difference under the replay, over all
    the logits of a step, is d = 0.8125.  The gate is not widened silently.  What is asserted instead:
      * decisions agree wherever the merged run's absolute top-2 gap is at least 2 d (both logits of a pair move by at most
        d, so only below that can a decision flip), with d measured here and held to the recorded value with 25 % headroom.
        That gate alone is weak: it covers 41 of the 356 decisions;
      * so the agreement itself is held to the record too: 9 of the 356 decisions differ (25 % headroom for the placement
        of ties: at most 11), and no miss has an absolute gap above the recorded largest, 0.125.  A wrong bank entry (another
        layer's or projection's pair) moves the logits by whole units and fails all three."""
    r = merged_vs_unmerged()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "multi_adapter_parity.json")) as f:
        rec = json.load(f)
    d = max(r["logit_diff"])
    free = free_decisions(PARITY_STEPS)
    safe = free & (r["gaps"] >= 2 * d)
    differ = free & (r["dec"] != r["gen"])
    below = free & (r["margins"] < PARITY_GATE)
    print("d %.6f (recorded %.6f), decisions %d, differ %d (recorded %d), largest gap of a miss %.6f (recorded %.6f); gap < 2 d: %d, misses above "
          "2 d %d; relative gate %.3f: below %d, misses above %d" %
          (d, rec["max_abs_logit_diff"], int(free.sum()), int(differ.sum()), rec["differing"], float(r["gaps"][differ].max(initial=0)),
           rec["max_miss_gap"], int((free & ~safe).sum()), int((differ & safe).sum()), PARITY_GATE, int(below.sum()), int((differ & ~below).sum())))
    assert below.sum() <= 0.1 * free.sum(), int(below.sum())
    assert d <= 1.25 * rec["max_abs_logit_diff"], (d, rec["max_abs_logit_diff"])
    assert not (differ & safe).any(), np.argwhere(differ & safe)[:10]
    assert differ.sum() <= 1.25 * rec["differing"], int(differ.sum())
    assert (r["gaps"][differ] <= rec["max_miss_gap"]).all(), r["gaps"][differ]
    assert np.array_equal(r["dec"][~free], r["gen"][~free])


# ---- 7. state rules -------------------------------------------------------------------------------------------------------------------
def test_bank_state_and_argument_errors():
    from mtts.engine import Engine
    eng = _engine(True)
    try:
        ids, mask = _prompts((21, 30), 8)
        name = _name(0, "self_attn.q_proj")
        A, B = _adapter(1)[name]
        a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()

        def load(idx=3, nm=name, rows=B.shape[0], cols=A.shape[1], r=RANK):
            return eng.lib.mtts_adapter_load(eng._h, idx, nm.encode(), a.data_ptr(), b.data_ptr(), rows, cols, r, C.c_float(SCALING), None)

        def err():
            return eng.lib.mtts_last_error().decode()

        want = _run(eng, ids, mask, 12, GREEDY, row_adapters=[0, -1])[0]
        # a run is open: the bank cannot change, and is as it was
        eng.begin(ids, mask, ids.shape[1] + 40, row_adapters=[0, -1])
        eng.step(5)
        assert load() == capi.ESTATE and eng.lib.mtts_adapter_clear(eng._h, 0) == capi.ESTATE
        eng.step(7)
        eng.sync_state()
        assert np.array_equal(eng.read_generated(12), want)
        eng.sched_open(4, 64)
        # arguments, each with the offending value in the message
        assert load(idx=16) == capi.EINVAL and "16" in err()
        assert load(idx=-1) == capi.EINVAL
        assert load(r=65) == capi.EINVAL and "65" in err()
        assert load(r=0) == capi.EINVAL
        assert load(rows=B.shape[0] - 32) == capi.EINVAL and str(B.shape[0] - 32) in err()
        for nm in ("model.language_model.layers.0.input_layernorm.weight", "model.embedding_list.1.weight", "lm_heads.0.weight",
                   "model.language_model.layers.0.self_attn.x_proj.weight", _name(NL, "self_attn.q_proj")):
            assert load(nm=nm) == capi.EINVAL, nm
        assert eng.lib.mtts_adapter_clear(eng._h, 16) == capi.EINVAL
        # an id that names an empty adapter: refused at begin, and the pending list is consumed by the failing call
        with pytest.raises(capi.MttsError) as ei:
            eng.begin(ids, mask, ids.shape[1] + 40, row_adapters=[3, -1])
        assert ei.value.code == capi.EINVAL and "adapter 3 is empty" in str(ei.value)
        assert np.array_equal(_run(eng, ids, mask, 12, GREEDY)[0], _run(eng, ids, mask, 12, GREEDY, row_adapters=[-1, -1])[0])
        three = np.array([0, 0, 0], np.int32)               # one id per prompt
        capi.check(eng.lib.mtts_set_row_adapters(eng._h, three.ctypes.data, 3))
        with pytest.raises(capi.MttsError) as ei:
            eng.begin(ids, mask, ids.shape[1] + 40)
        assert ei.value.code == capi.EINVAL and "3 ids" in str(ei.value)
        assert np.array_equal(_run(eng, ids, mask, 12, GREEDY, row_adapters=[0, -1])[0], want)      # nothing was left pending
        # a scheduler slot
        eng.sched_open(4, 64)
        p = _plain_prompt(np.random.default_rng(1), 40)
        with pytest.raises(capi.MttsError) as ei:
            eng.submit(0, p, p.shape[0] + 20, adapter=3)
        assert ei.value.code == capi.EINVAL
        eng.submit(0, p, p.shape[0] + 20)                   # the refused submit consumed the slot's adapter
        eng.sched_open(4, 64)
        # mtts_score takes no row adapters: refused while a list is pending, and the list stays for the next begin
        sid = np.full((2, 20, 8), 1024, dtype=np.int64)
        sid[:, :, 0] = 7
        two = np.array([0, -1], np.int32)
        capi.check(eng.lib.mtts_set_row_adapters(eng._h, two.ctypes.data, 2))
        with pytest.raises(capi.MttsError) as ei:
            eng.score(sid, np.ones((2, 20), np.uint8), sid)
        assert ei.value.code == capi.ESTATE
        assert np.array_equal(_run(eng, ids, mask, 12, GREEDY)[0], want)        # the pending list was this begin's
        assert np.isfinite(eng.score(sid, np.ones((2, 20), np.uint8), sid)[:, 1:]).all()
        # clearing: the adapter is empty again; loading a pair makes it usable
        eng.clear_bank_adapter(0)
        with pytest.raises(capi.MttsError):
            eng.begin(ids, mask, ids.shape[1] + 40, row_adapters=[0, -1])
        assert load(idx=0) == 0
        eng.begin(ids, mask, ids.shape[1] + 40, row_adapters=[0, -1])
        eng.sched_open(4, 64)
    finally:
        eng.close()
    # fp32 / fp16 engines have no bank, and say so
    for dtype in ("fp32", "fp16"):
        e32 = Engine(CFG, max_batch=2, max_seq_len=128, dtype=dtype)
        try:
            t = torch.zeros(RANK * 256, dtype=torch.float32, device="cuda")
            rc = e32.lib.mtts_adapter_load(e32._h, 0, name.encode(), t.data_ptr(), t.data_ptr(), 512, 256, RANK, C.c_float(1.0), None)
            assert rc == capi.EINVAL and "bf16 engine only" in e32.lib.mtts_last_error().decode() and dtype in e32.lib.mtts_last_error().decode()
            none = np.array([-1], np.int32)
            assert e32.lib.mtts_set_row_adapters(e32._h, none.ctypes.data, 1) == capi.EINVAL
            assert e32.lib.mtts_set_slot_adapter(e32._h, 0, 0) == capi.EINVAL
        finally:
            e32.close()


# ---- 8. model level -------------------------------------------------------------------------------------------------------------------
def test_generate_adapter_names_equals_single_prompt_calls():
    import modeling_asteroid as ma
    m = ma.AsteroidTTSInstruct.from_state_dict(CFG, _weights(), dtype="bf16").eval().to("cuda")
    try:
        m.load_adapter(_adapter(1), scaling=SCALING, adapter_name="x")
        ids, mask = _prompts((21, 40, 33), 9)
        ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
        base = m.generate(ids, mask, max_new_tokens=16).numpy()            # builds the engine: "x" is applied to it
        m.load_adapter(_adapter(2), scaling=SCALING, adapter_name="y")     # ... and "y" goes onto the resident engine
        names = ["x", "__base__", "y"]
        got = m.generate(ids, mask, max_new_tokens=16, adapter_names=names).numpy()
        assert np.array_equal(got[1], base[1]) and not np.array_equal(got[0], base[0]) and not np.array_equal(got[2], base[2])
        for b in range(3):
            one = m.generate(ids[b:b + 1], mask[b:b + 1], max_new_tokens=16, adapter_names=[names[b]]).numpy()
            assert np.array_equal(one[0], got[b]), b
        assert np.array_equal(m.generate(ids, mask, max_new_tokens=16, adapter_names=[None] * 3).numpy(), base)
        # num_return_sequences: row b * n + j is take j of prompt b, with prompt b's adapter
        m.generation_config.do_samples, m.generation_config.layers = SAMPLED[1], SAMPLED[0]
        out = m.generate(ids, mask, max_new_tokens=16, seed=5, num_return_sequences=2, adapter_names=names, return_dict_in_generate=True,
                         output_scores=True)
        assert out.sequences.shape[0] == 6
        for b in range(3):
            m.sample_rows = [b]
            one = m.generate(ids[b:b + 1], mask[b:b + 1], max_new_tokens=16, seed=5, num_return_sequences=2, adapter_names=[names[b]],
                             return_dict_in_generate=True, output_scores=True)
            m.sample_rows = None
            for j in range(2):
                assert np.array_equal(one.sequences[j].numpy(), out.sequences[2 * b + j].numpy()), (b, j)
                assert np.array_equal(np.nan_to_num(one.transition_scores[j].numpy()), np.nan_to_num(out.transition_scores[2 * b + j].numpy()))
        # a merged adapter and a named one compose: the delta adds to whatever weights are bound
        m.load_adapter(_adapter(2), scaling=SCALING)
        m.generation_config.do_samples, m.generation_config.layers = None, None
        both = m.generate(ids, mask, max_new_tokens=16, adapter_names=names).numpy()
        assert not np.array_equal(both[1], base[1]) and not np.array_equal(both[0], got[0])
        m.unload_adapter()
        m.delete_adapter("y")
        assert m.adapter_names() == ["x"]
        with pytest.raises(ValueError):
            m.generate(ids, mask, max_new_tokens=16, adapter_names=names)
        assert np.array_equal(m.generate(ids, mask, max_new_tokens=16, adapter_names=["x", None, None]).numpy()[0], got[0])
    finally:
        if m._engine is not None:
            m._engine.close()
