"""typical_p (HF's TypicalLogitsWarper, locally typical sampling) in the device sampler, on both sampler paths.  -m gpu.

The reference is HF itself (tests/typical_ref.py: the installed transformers' warpers on CPU torch, TypicalLogitsWarper
included, on the same bf16-rounded rows, behind the oracle's repetition penalty).  The kernel-level rows are boundary-safe
as that file's docstring says: doubt mass zero (no token whose membership HF's own fp32 noise could flip), the top-k /
top-p cuts and the floors as in test_sampler_floors_gpu.py.  On the in-block path every check is exact and lp is held to
scores_ref.KERNEL_TOL; the full-vocabulary path gets the allowances test_kernel_vs_hf_warpers grants it: the pick's CDF
interval holds u within 1e-4 of mass, lp gets 1e-4 over the kept mass more.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth, warp_spec  # noqa: E402
from mtts.engine import sampler_cfgs, sampler_floors, sampler_typical  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import floors_ref as fr  # noqa: E402
import scores_ref as sr  # noqa: E402
import typical_ref as tr  # noqa: E402

TOL = sr.KERNEL_TOL


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


class _Rows:
    """Logits and history bitmaps of one case on the device, uploaded once; sample() is one hook call."""

    def __init__(self, logits, hist, V, mask_id, channel):
        self.rows, self.V = logits.shape[0], V
        self.lt = torch.from_numpy(np.array(logits, dtype=np.float32)).to(torch.bfloat16).cuda()
        bm = np.zeros((self.rows, (V + 31) // 32), dtype=np.uint32)
        for b in range(self.rows):
            for t in hist[b]:
                bm[b, t >> 5] |= np.uint32(1 << (t & 31))
        self.bm = torch.from_numpy(bm.view(np.int32)).cuda()
        self.mask_id, self.channel = mask_id, channel
        self.all_banned = torch.full((self.rows, (V + 31) // 32), -1, dtype=torch.int32, device="cuda")

    def sample(self, lc, step, typical="layer", lp=True, hook="typical", seed=tr.SEED, ban=False):
        """typical: "layer" (lc's typical_p) or a number.  hook "bans": mtts_k_sample_bans, which has no typical_p.
        -> (tokens int64, lp or None)"""
        lib = capi.lib()
        cfg = sampler_cfgs([lc] * 8, [True] * 8)[0]
        tok = torch.full((self.rows,), -7, dtype=torch.int32, device="cuda")
        lpt = torch.full((self.rows,), 7.0, dtype=torch.float32, device="cuda") if lp else None
        arr = sampler_floors([lc] * 8, [True] * 8)
        fl = None if arr is None else C.byref(arr[0])
        args = (self.lt.data_ptr(), self.rows, self.V, self.bm.data_ptr(), C.byref(cfg), self.mask_id, C.c_uint64(seed), step,
                self.channel, tok.data_ptr(), lpt.data_ptr() if lp else None, fl, self.all_banned.data_ptr() if ban else None)
        if hook == "bans":
            capi.check(lib.mtts_k_sample_bans(*args, None))
        else:
            t = warp_spec.typical_of(lc) if typical == "layer" else float(typical)
            capi.check(lib.mtts_k_sample_typical(*args, C.c_float(t), None))
        torch.cuda.synchronize()
        return tok.cpu().numpy().astype(np.int64), (lpt.cpu().numpy() if lp else None)


def _case_rows(V, mode):
    logits, hist, want, doubt, _ = tr.case(V, mode)
    return _Rows(logits, hist, V, tr.VOCABS[V]["mask_id"], tr.VOCABS[V]["channel"]), want, doubt


# ---- 1. the kernels against HF ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(tr.MODES))
@pytest.mark.parametrize("V", list(tr.VOCABS))
def test_kernel_vs_hf_typical(V, mode):
    """6 rows x 6 steps per case, through mtts_k_sample_typical.  The pick lies in HF's kept set and is the token
    oracle.sample_from_scores draws from HF's processed row with the same (seed, step, row, channel); lp is within 2e-5 of
    the float64 log-softmax of that row; a second call gives the same bits; without lp the tokens are the same.
    V = 1 025 is the in-block path (top_k: behind the prefilter); V = 152 697 the full-vocabulary path without top_k or with
    6 000, the in-block one with 50.  On the full-vocabulary path, as in test_kernel_vs_hf_warpers: the pick must be the
    token whose CDF interval holds u within 1e-4 of mass, and lp gets typical_ref.lp_extra more."""
    lc = tr.MODES[mode]
    dev, want, doubt = _case_rows(V, mode)
    full = fr.full_path(V, lc)
    assert (doubt == 0.0).all() if V <= fr.SAMP_CAND else (doubt <= tr.DOUBT_CAP).all()
    tol = TOL + tr.lp_extra(V, lc)
    worst, mism, left = 0.0, 0, 0
    pre = tr.hf_scores(*tr.case(V, mode)[:2], lc, dev.mask_id, upto_typical=True)        # the rows HF's typical warper sees
    for b in range(tr.ROWS):
        left += int(not np.isfinite(want[b, int(np.argmax(pre[b]))]))
    for step in range(tr.STEPS):
        tok, lp = dev.sample(lc, step)
        tok2, lp2 = dev.sample(lc, step)
        assert np.array_equal(tok, tok2) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32))
        assert np.array_equal(dev.sample(lc, step, lp=False)[0], tok)
        draw = ao.sample_from_scores(want, tr.SEED, step, dev.channel)
        for b in range(tr.ROWS):
            assert 0 <= tok[b] < V and np.isfinite(want[b, tok[b]]), (mode, V, step, b, int(tok[b]))      # inside HF's kept set
            if full:
                kept = np.nonzero(np.isfinite(want[b]))[0]
                kept = kept[np.lexsort((kept, want[b][kept]))[::-1]]
                e = np.exp((want[b][kept] - want[b][kept].max()).astype(np.float32)).astype(np.float64)
                cum = np.cumsum(e) / e.sum()
                u = float(ao.philox_uniform(tr.SEED, step, b, dev.channel))
                j = int(np.nonzero(kept == tok[b])[0][0])
                lo = cum[j - 1] if j else 0.0
                assert lo - 1e-4 <= u <= cum[j] + 1e-4, (mode, V, step, b, lo, u, cum[j])
                mism += int(tok[b] != draw[b])
            else:
                assert tok[b] == draw[b], (mode, V, step, b, int(tok[b]), int(draw[b]))
            ref = sr.log_softmax64(want[b], tok[b])
            worst = max(worst, abs(float(lp[b]) - ref))
            assert abs(float(lp[b]) - ref) <= tol, (mode, V, step, b, float(lp[b]), ref, tol)
    print(f"typical {mode} V={V}: kept {np.isfinite(want).sum(-1).tolist()}, raw argmax left on {left} of {tr.ROWS} rows, "
          f"max |lp - fp64| = {worst:.3e} (tolerance {tol:.3e}), {mism} draws moved inside the mass allowance")
    if mode == "typ02":
        assert left > 0             # the one warper that removes the mode: the case must show it


# ---- 2. hand-built rows -------------------------------------------------------------------------------------------------
# V = 4 101: the smallest size class that takes the scan / collect / full kernels, and no multiple of 8
HAND_V = (1025, 4101)


def _hand(V, row):
    """One fp32 row (bf16-exact values) as 3 identical rows on the device; the last id is the masked one."""
    logits = np.repeat(np.asarray(row, dtype=np.float32)[None], 3, 0)
    assert np.array_equal(ao.round_bf16(logits), logits)
    return _Rows(logits, np.zeros((3, 0), dtype=np.int64), V, V - 1, 0 if V > fr.SAMP_CAND else 3)


@pytest.mark.parametrize("V", HAND_V)
def test_the_mode_leaves(V):
    """One token just below p = 0.5 over a uniform rest, typical_p = 0.3: the rest is closer to the entropy than the mode
    (shift p * D against (1 - p) * D), so the rest stays -- whole, it is one tie group -- and the mode leaves.  64 steps never
    return it and lp = -ln(kept count)."""
    n = V - 2                                        # the uniform rest (the mode and the masked id aside)
    top = float(ao.round_bf16(np.array([np.log(n) - 0.02], dtype=np.float32))[0])
    assert top < np.log(n) - 0.005                   # p(mode) < 0.5 with a margin the fp32 shifts resolve
    row = np.zeros(V, dtype=np.float32)
    row[7] = top
    dev = _hand(V, row)
    lc = dict(typical_p=0.3)
    spec = warp_spec.apply_floors(np.where(np.arange(V) == V - 1, -np.inf, row)[None], lc)[0]
    assert not np.isfinite(spec[7]) and np.isfinite(spec).sum() == n
    for step in range(64):
        tok, lp = dev.sample(lc, step)
        assert (tok != 7).all() and (tok != V - 1).all(), (V, step, tok)
        assert np.abs(lp.astype(np.float64) + np.log(n)).max() <= TOL, (V, step, lp, -np.log(n))
    # without typical_p the mode is drawn about every other time
    assert sum(int((dev.sample(dict(), step)[0] == 7).sum()) for step in range(16)) > 8


@pytest.mark.parametrize("V", HAND_V)
def test_uniform_row_stays_whole(V):
    """Every shift is 0: everything stays, the draw is the plain sampler's and lp = -ln(V - 1)."""
    dev = _hand(V, np.zeros(V, dtype=np.float32))
    for tp in (0.2, 0.9):
        for step in range(4):
            tok, lp = dev.sample(dict(typical_p=tp), step)
            t0, l0 = dev.sample(dict(), step)
            assert np.array_equal(tok, t0) and np.array_equal(lp.view(np.uint32), l0.view(np.uint32))
            assert np.abs(lp.astype(np.float64) + np.log(V - 1)).max() <= TOL


@pytest.mark.parametrize("V", HAND_V)
def test_tie_group_on_the_crossing_stays_whole(V):
    """Three levels: one token at 8, forty tied at 5, the rest at 0.  The tied group is the closest to the entropy and a
    part of it would reach typical_p: it stays whole and alone.  Picks over 32 steps cover only the group and lp = -ln 40."""
    row = np.zeros(V, dtype=np.float32)
    row[5] = 8.0
    grp = np.arange(100, 140)
    row[grp] = 5.0
    lc = dict(typical_p=0.1)
    masked = np.where(np.arange(V) == V - 1, -np.inf, row)
    spec = warp_spec.apply_floors(masked[None], lc)[0]
    assert np.array_equal(np.flatnonzero(np.isfinite(spec)), grp)
    p = np.exp(masked.astype(np.float64))
    p /= p.sum()
    assert p[grp[0]] < lc["typical_p"] < p[grp].sum() - p[grp[0]]             # the crossing falls inside the group
    want = tr.hf_process(masked[None], lc)[0]
    assert np.array_equal(np.isfinite(want), np.isfinite(spec))
    dev = _hand(V, row)
    seen = set()
    for step in range(32):
        tok, lp = dev.sample(lc, step)
        assert np.isin(tok, grp).all(), (V, step, tok)
        assert np.array_equal(tok, ao.sample_from_scores(np.repeat(want[None], 3, 0), tr.SEED, step, dev.channel))
        assert np.abs(lp.astype(np.float64) + np.log(40)).max() <= TOL
        seen.update(tok.tolist())
    assert len(seen) > 20


@pytest.mark.parametrize("V", HAND_V)
def test_all_banned_row_gives_token_0_and_nan(V):
    dev = _hand(V, np.zeros(V, dtype=np.float32))
    for lc in (dict(typical_p=0.5), dict(typical_p=0.5, top_k=50), dict(typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)):
        tok, lp = dev.sample(lc, 1, ban=True)
        assert np.array_equal(tok, np.zeros(3, dtype=np.int64)) and np.isnan(lp).all(), (V, lc, tok, lp)
    # the scratch those rows went through is clean
    assert np.isfinite(dev.sample(dict(typical_p=0.5), 0)[1]).all()


# ---- 3. absent is absent ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", list(tr.VOCABS))
def test_no_typical_is_the_bans_hook_bit_for_bit(V):
    """typical_p 0, 1.0 or a layer without one: tokens and lp are those of mtts_k_sample_bans, on the in-block path (top_k
    50 + top_p, with a floor) and on the full-vocabulary one (no top_k, with floors)."""
    dev, _, _ = _case_rows(V, "typ09")
    for lc in (dict(repetition_penalty=1.1, temperature=0.9, top_k=50, top_p=0.9, min_p=0.05),
               dict(repetition_penalty=1.2, temperature=1.3, min_p=0.02, eta_cutoff=2e-3), dict(temperature=0.9)):
        for step in range(3):
            tok, lp = dev.sample(lc, step, hook="bans")
            for typical in (0.0, 1.0, "layer"):
                t2, l2 = dev.sample(lc, step, typical=typical)
                assert np.array_equal(tok, t2) and np.array_equal(lp.view(np.uint32), l2.view(np.uint32)), (V, typical, step)
            assert np.array_equal(dev.sample(lc, step, typical=0.0, lp=False)[0], tok)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------
def test_hook_refuses_bad_typical():
    dev, _, _ = _case_rows(1025, "typ09")
    lib = capi.lib()
    cfg = sampler_cfgs([dict(temperature=0.9)] * 8, [True] * 8)[0]
    tok = torch.zeros(tr.ROWS, dtype=torch.int32, device="cuda")
    for bad in (1.5, -0.1, float("nan"), float("inf")):
        rc = lib.mtts_k_sample_typical(dev.lt.data_ptr(), tr.ROWS, 1025, dev.bm.data_ptr(), C.byref(cfg), 1024, C.c_uint64(1), 0, 3,
                                       tok.data_ptr(), None, None, None, C.c_float(bad), None)
        msg = lib.mtts_last_error().decode()
        assert rc == capi.EINVAL and "typical_p" in msg and "channel" in msg, (bad, rc, msg)


# ---- 5. the engine ------------------------------------------------------------------------------------------------------
# test_engine_floors_vs_hf_on_its_own_logits' scenario with mixed layers: channel 0 typical on the full-vocabulary path, the
# speech channels typical alone, behind top-k, with floors, not at all, and a greedy channel whose typical_p is ignored
TYP_LAYERS = ([dict(repetition_penalty=1.1, temperature=0.9, typical_p=0.9),
               dict(repetition_penalty=1.05, temperature=1.1, typical_p=0.5),
               dict(repetition_penalty=1.05, temperature=1.1, top_k=30, typical_p=0.7),
               dict(repetition_penalty=1.05, temperature=1.1, typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=2e-2),
               dict(repetition_penalty=1.05, temperature=1.1, top_p=0.95, min_p=0.02, typical_p=0.8),
               dict(repetition_penalty=1.05, temperature=1.1, top_k=30, top_p=0.95),
               dict(repetition_penalty=1.05, temperature=1.1, typical_p=0.2),
               dict(repetition_penalty=1.05, temperature=1.1, typical_p=0.5)],
              [True] * 7 + [False])
TYP_SEED = 6             # (with this seed a row flushes and leaves early in all three dtypes, row 0 runs ~40 steps, the run ~45)


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


def _stepped_run(eng, ids, mask, ml, layers, ds, seed, new, keep_logits=False, n=1):
    eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=seed, output_scores=True)
    plan = eng.step_plan(1)
    logs = []
    for _ in range(0, new + 16, n):          # (the run ends by itself: max_length, then at most two 7-step flushes)
        if keep_logits:
            logs.append(eng.read_logits())
        eng.step(n)
        _, done = eng.sync_state()
        if done:
            break
    return eng.read_generated(new + 16), eng.read_scores(new + 16), logs, plan


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp16"])
def test_engine_typical_vs_hf_on_its_own_logits(dtype):
    """Ragged B=3.  Per step read_logits() then step(1); lp is recomputed on the host with the HF warpers from those logits
    and the known history at the appended token: 2e-5, and at most 1 slot in 240 outside it (a token that fp32 noise
    moves across a cut: the allowance of test_engine_floors_vs_hf_on_its_own_logits).  The NaN pattern is the state
    machine's.  The run repeats bit for bit; step(4) runs equal step(1) runs; row 0 (no padding) has the tokens of its
    batch-1 run through the continuous batcher; the run that follows without typical_p is a fresh engine's run (a one-shot)
    and only the first run's plan says `typical`."""
    from mtts.scheduler import ContinuousBatcher
    sc, cfg, w, ids, mask = _scenario(dtype)
    layers, ds = TYP_LAYERS
    new = sc["new"]
    ml = ids.shape[1] + new
    base = ids.shape[1] - 7
    eng = _engine(cfg, w, dtype)
    gen, lp, logs, plan = _stepped_run(eng, ids, mask, ml, layers, ds, TYP_SEED, new, keep_logits=True)
    assert any(line.startswith("sample:") and "typical" in line.split() for line in plan), plan
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
                want, s = tr.expected_lp(row, history, layers[c], ds[c], g, c, int(gen[g, r, c]))
                n += 1
                dev = abs(float(lp[g, r, c]) - want) if np.isfinite(s[gen[g, r, c]]) else np.inf
                if dev > TOL:
                    over += 1
                else:
                    worst = max(worst, dev)
    print(f"engine typical {dtype}: {G} steps, {n} slots, max deviation within tolerance {worst:.3e}, {over} over")
    assert n > 400
    assert over <= n // 240, (over, n)
    # bit-identical when repeated, and in steps of 4
    gen2, lp2, _, _ = _stepped_run(eng, ids, mask, ml, layers, ds, TYP_SEED, new)
    assert _eq(gen2, gen) and np.array_equal(lp2.view(np.uint32), lp.view(np.uint32))
    gen2, lp2, _, _ = _stepped_run(eng, ids, mask, ml, layers, ds, TYP_SEED, new, n=4)
    assert _eq(gen2[:G], gen) and np.array_equal(lp2[:G].view(np.uint32), lp.view(np.uint32))
    # the run that follows without typical_p: a fresh engine's
    plain_layers = [tr.plain(lc) for lc in layers]
    gen3, lp3, _, plan3 = _stepped_run(eng, ids, mask, ml, plain_layers, ds, TYP_SEED, new)
    assert not any("typical" in line for line in plan3), plan3
    fresh = _engine(cfg, w, dtype)
    gen4, lp4, _, plan4 = _stepped_run(fresh, ids, mask, ml, plain_layers, ds, TYP_SEED, new)
    fresh.close()
    assert plan3 == plan4 and _eq(gen3, gen4) and np.array_equal(lp3.view(np.uint32), lp4.view(np.uint32))
    assert not _eq(gen3, gen)                                            # (typical_p did change the run)
    # row 0 alone through the continuous batcher, same layers
    cb = ContinuousBatcher(eng, slots=2, gen_cap=new + 16, layers=layers, do_samples=ds)
    assert any("typical" in line for line in eng.step_plan(1))
    res, scs = cb.run([ids[0]], new, seeds=[TYP_SEED], row_ids=[0], output_scores=True)
    g0 = res[0].shape[0] - base
    assert g0 >= 8 and _eq(res[0][base:], gen[:g0, 0]) and _eq(scs[0], lp[:g0, 0])
    # ... and the one-shot holds for the scheduler too
    ContinuousBatcher(eng, slots=2, gen_cap=new + 16, layers=plain_layers, do_samples=ds)
    assert not any("typical" in line for line in eng.step_plan(1))
    eng.close()


def test_engine_setter_one_shot_and_refusals():
    """mtts_set_sampler_typical: a refused table names the channel and leaves nothing pending; a table set before a begin
    that fails is consumed by it."""
    sc, cfg, w, ids, mask = _scenario("bf16")
    eng = _engine(cfg, w, "bf16")
    lib = capi.lib()
    layers, ds = TYP_LAYERS
    for bad in (1.5, -0.25, float("nan")):
        arr = sampler_typical(layers, ds)
        arr[5] = bad
        assert lib.mtts_set_sampler_typical(eng._h, arr) == capi.EINVAL
        assert "channel 5" in lib.mtts_last_error().decode() and "typical_p" in lib.mtts_last_error().decode()
    ml = ids.shape[1] + 12
    plain_layers = [fr.four(lc) for lc in layers]       # (the bare mtts_begin below sets no floors either)
    assert lib.mtts_set_sampler_typical(eng._h, sampler_typical(layers, ds)) == 0 and lib.mtts_set_sampler_typical(eng._h, None) == 0
    want = eng.generate(ids, mask, ml, layers=plain_layers, do_samples=ds, seed=3)
    capi.check(lib.mtts_set_sampler_typical(eng._h, sampler_typical(layers, ds)))
    m = np.ascontiguousarray((mask > 0).astype(np.uint8))
    i64 = np.ascontiguousarray(ids, dtype=np.int64)
    scfg = sampler_cfgs(plain_layers, ds)
    assert lib.mtts_begin(eng._h, i64.ctypes.data, m.ctypes.data, 3, 4, 64, scfg, C.c_uint64(3), None) == capi.EINVAL      # T < 8
    capi.check(lib.mtts_begin(eng._h, i64.ctypes.data, m.ctypes.data, 3, ids.shape[1], ml, scfg, C.c_uint64(3), None))
    eng._B = 3
    assert not any("typical" in line for line in eng.step_plan(1))
    for _ in range(ml):
        eng.step(4)
        if eng.sync_state()[1]:
            break
    got = eng.read_generated(ml + 64)
    base = ids.shape[1] - 7
    assert got.shape[0] == want.shape[1] - base and _eq(np.ascontiguousarray(got.transpose(1, 0, 2)), want[:, base:])
    # 0 and 1 are "absent": the plain run, the plain plan
    capi.check(lib.mtts_set_sampler_typical(eng._h, (C.c_float * 8)(0, 1, 0, 1, 0, 1, 0, 1)))
    assert _eq(eng.generate(ids, mask, ml, layers=plain_layers, do_samples=ds, seed=3), want)
    # the other way round: with typical_p the tokens differ
    assert not _eq(eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=3), want)
    eng.close()


# ---- 6. the model -------------------------------------------------------------------------------------------------------
def test_model_generate_typical_p():
    """generate(typical_p=0.5) is Engine.generate with the key in every channel's dict and differs from the run without it;
    typical_p=1.0 is the plain run; generation_config.typical_p is the keyword's default; two takes equal the
    repeat-interleaved batch."""
    from modeling_asteroid import AsteroidTTSInstruct, GenerationConfig
    sc = sr.SCENARIO
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, sc["weight_seed"], bf16=True, **sc["wkw"])
    four = dict(repetition_penalty=1.1, temperature=1.0, top_k=30, top_p=0.9)
    gc = GenerationConfig(do_sample=True, eos_token_id=cfg["eos_token_id"], **four)
    m = AsteroidTTSInstruct.from_state_dict(cfg, {k: torch.from_numpy(v) for k, v in w.items()}, gc).to("cuda")
    ids_np, mask_np = synth.synth_prompts(cfg, 41, 3, 40, 0.4, True)
    ids, mask = torch.from_numpy(ids_np), torch.from_numpy(mask_np)
    new = 24
    plain = m.generate(ids, mask, max_new_tokens=new, seed=5)
    got = m.generate(ids, mask, max_new_tokens=new, seed=5, typical_p=0.5)
    assert not torch.equal(got, plain)
    want = m._engine.generate(ids_np, mask_np, ids.shape[1] + new, layers=[dict(four, typical_p=0.5)] * 8, do_samples=[True] * 8, seed=5)
    assert _eq(got.cpu().numpy(), want)
    assert torch.equal(m.generate(ids, mask, max_new_tokens=new, seed=5, typical_p=1.0), plain)
    m.generation_config.typical_p = 0.5
    assert torch.equal(m.generate(ids, mask, max_new_tokens=new, seed=5), got)
    assert torch.equal(m.generate(ids, mask, max_new_tokens=new, seed=5, typical_p=1.0), plain)
    m.generation_config.typical_p = 1.0
    two = m.generate(ids, mask, max_new_tokens=new, seed=5, typical_p=0.5, num_return_sequences=2)
    rep = m.generate(ids.repeat_interleave(2, 0), mask.repeat_interleave(2, 0), max_new_tokens=new, seed=5, typical_p=0.5)
    assert two.shape[0] == 6 and torch.equal(two, rep)
