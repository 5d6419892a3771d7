"""Probability floors (min_p, epsilon_cutoff, eta_cutoff) in the device sampler.  -m gpu.

The reference is HF itself (tests/floors_ref.py: the installed transformers' warpers on CPU torch, on the same
bf16-rounded rows, behind the oracle's repetition penalty).  A token on a floor carries real mass, up to min_p * p_max, so
the kernel-level rows are boundary-safe: no token within 1e-3 (relative, float64) of a floor, and the top-k / top-p cuts
as in test_scores_gpu.py::test_kernel_lp_vs_fp64.  The lp tolerance is that test's 2e-5 budget (scores_ref.KERNEL_TOL):
the floors add no arithmetic to lp itself, which stays (s_d - smax) - log(sum over the kept set).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402
from mtts.engine import sampler_cfgs, sampler_floors  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import floors_ref as fr  # noqa: E402
import scores_ref as sr  # noqa: E402

TOL = sr.KERNEL_TOL


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


class _Rows:
    """Logits and history bitmaps of one case on the device, uploaded once; sample() is one hook call."""

    def __init__(self, logits, hist, V):
        self.rows, self.V = logits.shape[0], V
        self.lt = torch.from_numpy(np.array(logits, dtype=np.float32)).to(torch.bfloat16).cuda()          # (a copy: the case is read-only)
        bm = np.zeros((self.rows, (V + 31) // 32), dtype=np.uint32)
        for b in range(self.rows):
            for t in hist[b]:
                bm[b, t >> 5] |= np.uint32(1 << (t & 31))
        self.bm = torch.from_numpy(bm.view(np.int32)).cuda()
        self.mask_id, self.channel = fr.VOCABS[V]["mask_id"], fr.VOCABS[V]["channel"]

    def sample(self, lc, step, floors="layer", lp=True, hook="floors", seed=fr.SEED):
        """floors: "layer" (those of lc), None (a NULL pointer) or "zero" (a struct of zeros).  -> (tokens int64, lp or None)"""
        lib = capi.lib()
        cfg = sampler_cfgs([lc] * 8, [True] * 8)[0]
        tok = torch.full((self.rows,), -7, dtype=torch.int32, device="cuda")
        lpt = torch.full((self.rows,), 7.0, dtype=torch.float32, device="cuda") if lp else None
        args = (self.lt.data_ptr(), self.rows, self.V, self.bm.data_ptr(), C.byref(cfg), self.mask_id, C.c_uint64(seed), step,
                self.channel, tok.data_ptr(), lpt.data_ptr() if lp else None)
        if hook == "scores":
            capi.check(lib.mtts_k_sample_scores(*args, None))
        else:
            fl = None
            if floors == "zero":
                fl = C.byref(capi.MttsSamplerFloors())
            elif floors == "layer":
                arr = sampler_floors([lc] * 8, [True] * 8)
                fl = None if arr is None else C.byref(arr[0])
            capi.check(lib.mtts_k_sample_floors(*args, fl, None))
        torch.cuda.synchronize()
        return tok.cpu().numpy().astype(np.int64), (lpt.cpu().numpy() if lp else None)


# ---- 1. the kernels against HF ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(fr.MODES))
@pytest.mark.parametrize("V", list(fr.VOCABS))
def test_kernel_vs_hf_warpers(V, mode):
    """6 rows x 6 steps per case.  The pick lies in HF's kept set and is the token oracle.sample_from_scores draws from HF's
    processed row with the same (seed, step, row, channel); lp is within 2e-5 of the float64 log-softmax of that row; a
    second call gives the same bits; without lp the tokens are the same.
    Where top-p acts on the full-vocabulary path (no top_k, or top_k = 6000, on 152 697 tokens) which 1e-6-mass tokens sit on
    the nucleus boundary is fp32 noise in HF's own cumsum: there the pick must be the token whose CDF interval holds u
    within 1e-4 of mass (test_engine_gpu.py::test_sampler_kernel_vs_oracle) and lp gets 1e-4 / top_p more
    (test_scores_gpu.py::test_kernel_lp_vs_fp64)."""
    lc = fr.MODES[mode]
    logits, hist, want = fr.case(V, mode)
    dev = _Rows(logits, hist, V)
    nucleus_full = bool(fr.full_path(V, lc) and lc.get("top_p"))
    tol = TOL + (1e-4 / lc["top_p"] if nucleus_full else 0.0)
    worst, mism = 0.0, 0
    for step in range(fr.STEPS):
        tok, lp = dev.sample(lc, step)
        tok2, lp2 = dev.sample(lc, step)
        assert np.array_equal(tok, tok2) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32))
        assert np.array_equal(dev.sample(lc, step, lp=False)[0], tok)
        draw = ao.sample_from_scores(want, fr.SEED, step, dev.channel)
        for b in range(fr.ROWS):
            assert 0 <= tok[b] < V and np.isfinite(want[b, tok[b]]), (mode, V, step, b, int(tok[b]))      # inside HF's kept set
            if nucleus_full:
                kept = np.nonzero(np.isfinite(want[b]))[0]
                kept = kept[np.lexsort((kept, want[b][kept]))[::-1]]
                e = np.exp((want[b][kept] - want[b][kept].max()).astype(np.float32)).astype(np.float64)
                cum = np.cumsum(e) / e.sum()
                u = float(ao.philox_uniform(fr.SEED, step, b, dev.channel))
                j = int(np.nonzero(kept == tok[b])[0][0])
                lo = cum[j - 1] if j else 0.0
                assert lo - 1e-4 <= u <= cum[j] + 1e-4, (mode, V, step, b, lo, u, cum[j])
                mism += int(tok[b] != draw[b])
            else:
                assert tok[b] == draw[b], (mode, V, step, b, int(tok[b]), int(draw[b]))
            ref = sr.log_softmax64(want[b], tok[b])
            worst = max(worst, abs(float(lp[b]) - ref))
            assert abs(float(lp[b]) - ref) <= tol, (mode, V, step, b, float(lp[b]), ref, tol)
    print(f"floors {mode} V={V}: kept {np.isfinite(want).sum(-1).tolist()}, max |lp - fp64| = {worst:.3e} (tolerance {tol:.3e}), "
          f"{mism} draws moved inside the mass allowance")


@pytest.mark.parametrize("V", list(fr.VOCABS))
def test_no_floors_is_the_plain_sampler_bit_for_bit(V):
    """floors NULL, a struct of zeros, or a layer that sets none: tokens and lp are those of mtts_k_sample_scores, on the
    in-block path (top_k 50 + top_p) and on the full-vocabulary one (no top_k)."""
    logits, hist, _ = fr.case(V, "top_k_min_p")
    dev = _Rows(logits, hist, V)
    for lc in (dict(repetition_penalty=1.1, temperature=0.9, top_k=50, top_p=0.9), dict(repetition_penalty=1.2, temperature=1.3)):
        for step in range(3):
            tok, lp = dev.sample(lc, step, hook="scores")
            for floors in (None, "zero", "layer"):
                t2, l2 = dev.sample(lc, step, floors=floors)
                assert np.array_equal(tok, t2) and np.array_equal(lp.view(np.uint32), l2.view(np.uint32)), (V, floors, step)


@pytest.mark.parametrize("V", list(fr.VOCABS))
def test_min_p_one_is_the_argmax(V):
    """min_p = 1 on rows whose maximum is not shared: every other token is below p_max and leaves; lp = log(1) = 0."""
    rng = np.random.default_rng(77 + V % 97)
    for lc in (dict(repetition_penalty=1.1, temperature=0.9, min_p=1.0), dict(repetition_penalty=1.1, temperature=0.9, top_k=50, min_p=1.0)):
        rows = [fr.safe_row(rng, V, lc, fr.VOCABS[V]["mask_id"], tie_free=True) for _ in range(fr.ROWS)]
        logits, hist = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        lm = logits.copy()
        lm[:, fr.VOCABS[V]["mask_id"]] = -np.inf
        want = np.argmax(ao.apply_processors(hist, lm, dict(repetition_penalty=1.1, temperature=0.9)), -1)
        dev = _Rows(logits, hist, V)
        for step in range(2):
            tok, lp = dev.sample(lc, step)
            assert np.array_equal(tok, want) and np.array_equal(lp, np.zeros(fr.ROWS, dtype=np.float32)), (V, lc, tok, want, lp)


def test_hook_refuses_bad_floors():
    logits, hist, _ = fr.case(1025, "min_p")
    dev = _Rows(logits, hist, 1025)
    lib = capi.lib()
    cfg = sampler_cfgs([dict(temperature=0.9)] * 8, [True] * 8)[0]
    tok = torch.zeros(fr.ROWS, dtype=torch.int32, device="cuda")
    for bad, word in ((dict(min_p=1.5), "min_p"), (dict(epsilon_cutoff=1.0), "epsilon_cutoff"), (dict(eta_cutoff=-0.1), "eta_cutoff"),
                      (dict(min_p=float("nan")), "min_p")):
        fl = capi.MttsSamplerFloors(**bad)
        rc = lib.mtts_k_sample_floors(dev.lt.data_ptr(), fr.ROWS, 1025, dev.bm.data_ptr(), C.byref(cfg), 1024, C.c_uint64(1), 0, 3,
                                      tok.data_ptr(), None, C.byref(fl), None)
        assert rc == capi.EINVAL and word in lib.mtts_last_error().decode()


# ---- 2. the engine ----------------------------------------------------------------------------------------------------------
# test_scores_gpu.py::test_engine_lp_vs_its_own_logits' scenario with mixed floors: channel 0 without top_k (the
# full-vocabulary kernel, min_p then eta), the speech channels on the in-block path with one floor, two, all three, none, and
# a greedy channel whose floor must be ignored
FLOOR_LAYERS = ([dict(repetition_penalty=1.1, temperature=0.9, min_p=0.05, eta_cutoff=2e-3),
                 dict(repetition_penalty=1.05, temperature=1.1, top_k=30, top_p=0.95, min_p=0.1),
                 dict(repetition_penalty=1.05, temperature=1.1, epsilon_cutoff=3e-3),
                 dict(repetition_penalty=1.05, temperature=1.1, top_k=30, eta_cutoff=2e-2),
                 dict(repetition_penalty=1.05, temperature=1.1, top_p=0.95, min_p=0.02, epsilon_cutoff=3e-4, eta_cutoff=2e-3),
                 dict(repetition_penalty=1.05, temperature=1.1, top_k=30, top_p=0.95),
                 dict(repetition_penalty=1.05, temperature=1.1, min_p=0.3),
                 dict(repetition_penalty=1.05, temperature=1.1, min_p=0.5)],
                [True] * 7 + [False])
FLOOR_SEED = 10           # (the floors change the draws: with the scenario's own seed no bf16 row reaches an EOS; with this one
                          #  a row flushes and leaves early in all three dtypes and the run still takes ~50 steps)


def _scenario(dtype):
    sc = sr.SCENARIO
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, sc["weight_seed"], bf16=(dtype == "bf16"), **sc["wkw"])
    ids, mask = synth.synth_prompts(cfg, sc["prompt_seed"], sc["batch"], sc["prompt_len"], sc["audio_frac"], True)
    return sc, cfg, w, ids, mask


def _engine(cfg, w, dtype):
    from mtts.engine import Engine
    eng = Engine(cfg, max_batch=4, max_seq_len=256, dtype=dtype)
    eng.bind_state_dict(w)
    return eng


def _stepped_run(eng, ids, mask, ml, layers, ds, seed, new, keep_logits=False):
    eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=seed, output_scores=True)
    plan = eng.step_plan(1)
    logs = []
    for _ in range(new + 8):
        if keep_logits:
            logs.append(eng.read_logits())
        eng.step(1)
        _, done = eng.sync_state()
        if done:
            break
    return eng.read_generated(new + 16), eng.read_scores(new + 16), logs, plan


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp16"])
def test_engine_floors_vs_hf_on_its_own_logits(dtype):
    """Ragged B=3, ~50 steps, one row runs an EOS flush and leaves early.  Per step read_logits() then step(1); lp is
    recomputed on the host with the HF warpers from those logits and the known history at the appended token: 2e-5, and at
    most 1 slot in 240 outside it (a token that fp32 noise moves across a cut: the allowance of
    test_engine_lp_vs_its_own_logits).  The NaN pattern is the state machine's.  The run repeats bit for bit; row 0 (no
    padding) has the tokens of its batch-1 run through the continuous batcher; the run that follows without floors is a
    fresh engine's run (the floors are a one-shot) and only the first run's plan says `floors`."""
    from mtts.scheduler import ContinuousBatcher
    sc, cfg, w, ids, mask = _scenario(dtype)
    layers, ds = FLOOR_LAYERS
    new = sc["new"]
    ml = ids.shape[1] + new
    base = ids.shape[1] - 7
    eng = _engine(cfg, w, dtype)
    gen, lp, logs, plan = _stepped_run(eng, ids, mask, ml, layers, ds, FLOOR_SEED, new, keep_logits=True)
    assert any(line.startswith("sample:") and "floors" in line.split() for line in plan), plan
    G = gen.shape[0]
    assert lp.shape == gen.shape and G >= 40
    used = sr.used_mask(gen, base, ml, cfg)
    assert np.array_equal(np.isnan(lp), ~used)
    per_row = used.sum((0, 2))
    assert per_row.min() < per_row.max() and (gen[:, :, 0] == cfg["eos_token_id"]).any()      # a row flushed and left early
    worst, over, n = 0.0, 0, 0
    for g in range(G):
        l0, l17 = logs[g]
        for r in range(3):
            for c in range(8):
                if not used[g, r, c]:
                    continue
                row = l0[r] if c == 0 else l17[c - 1, r]
                history = np.concatenate([ids[r, :base, c], gen[:g, r, c]])
                want, s = fr.expected_lp(row, history, layers[c], ds[c], g, c, int(gen[g, r, c]))
                n += 1
                dev = abs(float(lp[g, r, c]) - want) if np.isfinite(s[gen[g, r, c]]) else np.inf
                if dev > TOL:
                    over += 1
                else:
                    worst = max(worst, dev)
    print(f"engine floors {dtype}: {n} slots, max deviation within tolerance {worst:.3e}, {over} over")
    assert n > 400
    assert over <= n // 240, (over, n)
    # bit-identical when repeated
    gen2, lp2, _, _ = _stepped_run(eng, ids, mask, ml, layers, ds, FLOOR_SEED, new)
    assert _eq(gen2, gen) and np.array_equal(lp2.view(np.uint32), lp.view(np.uint32))
    # the run that follows without floors: a fresh engine's
    plain_layers = [fr.four(lc) for lc in layers]
    gen3, lp3, _, plan3 = _stepped_run(eng, ids, mask, ml, plain_layers, ds, FLOOR_SEED, new)
    assert not any("floors" in line for line in plan3), plan3
    fresh = _engine(cfg, w, dtype)
    gen4, lp4, _, plan4 = _stepped_run(fresh, ids, mask, ml, plain_layers, ds, FLOOR_SEED, new)
    fresh.close()
    assert plan3 == plan4 and _eq(gen3, gen4) and np.array_equal(lp3.view(np.uint32), lp4.view(np.uint32))
    assert not _eq(gen3, gen)                                            # (the floors did change the run)
    # row 0 alone through the continuous batcher, same layers
    cb = ContinuousBatcher(eng, slots=2, gen_cap=new + 16, layers=layers, do_samples=ds)
    assert any("floors" in line for line in eng.step_plan(1))
    res, scs = cb.run([ids[0]], new, seeds=[FLOOR_SEED], row_ids=[0], output_scores=True)
    g0 = res[0].shape[0] - base
    assert g0 >= 8 and _eq(res[0][base:], gen[:g0, 0]) and _eq(scs[0], lp[:g0, 0])
    # ... and the one-shot holds for the scheduler too
    ContinuousBatcher(eng, slots=2, gen_cap=new + 16, layers=plain_layers, do_samples=ds)
    assert not any("floors" in line for line in eng.step_plan(1))
    eng.close()


def test_engine_setter_one_shot_and_refusals():
    """mtts_set_sampler_floors: a refused table names the channel and leaves nothing pending; floors set before a begin
    that fails are consumed by it."""
    sc, cfg, w, ids, mask = _scenario("bf16")
    eng = _engine(cfg, w, "bf16")
    lib = capi.lib()
    layers, ds = FLOOR_LAYERS
    arr = sampler_floors(layers, ds)
    arr[5].epsilon_cutoff = 1.0
    assert lib.mtts_set_sampler_floors(eng._h, arr) == capi.EINVAL
    assert "channel 5" in lib.mtts_last_error().decode() and "epsilon_cutoff" in lib.mtts_last_error().decode()
    ml = ids.shape[1] + 12
    plain_layers = [fr.four(lc) for lc in layers]
    want = eng.generate(ids, mask, ml, layers=plain_layers, do_samples=ds, seed=3)
    capi.check(lib.mtts_set_sampler_floors(eng._h, sampler_floors(layers, ds)))
    m = np.ascontiguousarray((mask > 0).astype(np.uint8))
    i64 = np.ascontiguousarray(ids, dtype=np.int64)
    scfg = sampler_cfgs(plain_layers, ds)
    assert lib.mtts_begin(eng._h, i64.ctypes.data, m.ctypes.data, 3, 4, 64, scfg, C.c_uint64(3), None) == capi.EINVAL      # T < 8
    capi.check(lib.mtts_begin(eng._h, i64.ctypes.data, m.ctypes.data, 3, ids.shape[1], ml, scfg, C.c_uint64(3), None))
    eng._B = 3
    assert not any("floors" in line for line in eng.step_plan(1))
    for _ in range(ml):
        eng.step(4)
        if eng.sync_state()[1]:
            break
    got = eng.read_generated(ml + 64)
    base = ids.shape[1] - 7
    assert got.shape[0] == want.shape[1] - base and _eq(np.ascontiguousarray(got.transpose(1, 0, 2)), want[:, base:])
    # the other way round: with floors the tokens differ
    assert not _eq(eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=3), want)
    eng.close()
