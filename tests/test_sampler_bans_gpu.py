"""Hard bans (no_repeat_ngram_size, suppress_tokens, min_new_tokens) on the device.  -m gpu.

The reference is HF itself (tests/bans_ref.py: the installed transformers' processors on CPU torch) and mtts/ban_spec.py,
which tests/test_sampler_bans_cpu.py holds against them.  The bans add no arithmetic to the sampler -- a banned token is a
token at -inf -- so the lp budget is that of the sampler without them (scores_ref.KERNEL_TOL).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import ban_spec, capi, synth  # noqa: E402
from mtts.engine import Engine, sampler_cfgs, sampler_floors  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import bans_ref as br  # noqa: E402
import floors_ref as fr  # noqa: E402
import scores_ref as sr  # noqa: E402

TOL = sr.KERNEL_TOL
BAN_T = 256               # csrc/sampler.hip: threads of a ban block = the stride of its window scan


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- 1. the ban kernel against ban_spec, exact ----------------------------------------------------------------------------
def _ban_kernel(hists, n, static, V, eos=None, out=None, cap=None):
    """hists: list of 1-D int arrays -> uint32 [rows, ceil(V/32)] from mtts_k_ngram_ban; `out`: a device buffer to reuse."""
    rows = len(hists)
    cap = max([len(h) for h in hists] + [1]) if cap is None else cap
    hm = np.full((rows, cap), -3, dtype=np.int32)
    for r, h in enumerate(hists):
        hm[r, :len(h)] = h
    dh = torch.from_numpy(hm).cuda()
    dl = torch.tensor([len(h) for h in hists], dtype=torch.int32, device="cuda")
    words = (V + 31) // 32
    if out is None:
        out = torch.full((rows, words), -1, dtype=torch.int32, device="cuda")        # (stale bits everywhere: the kernel overwrites)
    st = (C.c_int32 * max(len(static), 1))(*static)
    capi.check(capi.lib().mtts_k_ngram_ban(dh.data_ptr(), dl.data_ptr(), rows, cap, n, st, len(static), V,
                                           -1 if eos is None else eos, 0 if eos is None else 1, out.data_ptr(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), out


def _want_words(hists, n, static, V, eos=None):
    layer = dict(no_repeat_ngram_size=n, suppress_tokens=static, min_new_tokens=1 if eos is not None else 0)
    return np.stack([ban_spec.ban_words(ban_spec.banned_mask(h, 0, V, layer, eos_token_id=eos)) for h in hists])


@pytest.mark.parametrize("V", [1025, 152697])
@pytest.mark.parametrize("n", [1, 2, 3, 16])
def test_ban_kernel_is_ban_spec(V, n):
    """Lengths 0, n-1, n, n+1, the block stride +- 1 (in windows and in tokens) and 8 200, alphabets of 3..6 symbols spread
    over the vocabulary (token V-1 among them: the last word), with and without the static list and eos; a match only at
    window 0, only at the last window, and a periodic history where every window matches.  Exact, and bits at and above V
    stay 0 although the output buffer starts as all ones."""
    rng = np.random.default_rng(40 * n + V % 97)
    lens = sorted({0, max(n - 1, 0), n, n + 1, BAN_T - 1, BAN_T, BAN_T + 1, BAN_T + n - 2, BAN_T + n - 1, BAN_T + n, 8200})
    hists = []
    for L in lens:
        alphabet = np.concatenate([rng.choice(V - 1, int(rng.integers(2, 6)), replace=False), [V - 1]])
        hists.append(rng.choice(alphabet, L))
    # distinct tokens except one repeat of the suffix: at window 0, and at the last window len - n
    L = 700
    base = rng.choice(V, L, replace=False)
    first, last = base.copy(), base.copy()
    if n > 1:
        first[:n - 1] = first[L - n + 1:]       # the suffix once more in front: window 0 matches, its follower first[n-1] goes
        last[L - n:] = last[L - 1]              # a run of n equal tokens at the end: window L-n alone matches
    hists += [first, last, np.tile(rng.choice(V, 3, replace=False), 400)[:1000], np.full(900, V - 1)]
    for static, eos in (([], None), (br.SUPPRESS, None), (br.SUPPRESS, 999)):
        got, _ = _ban_kernel(hists, n, static, V, eos)
        want = _want_words(hists, n, static, V, eos)
        assert got.shape == want.shape
        bad = np.argwhere(got != want)
        assert bad.size == 0, (V, n, static, eos, bad[:5], [len(hists[i]) for i in np.unique(bad[:5, 0])])
    # the constructed rows ban exactly what they were built to ban
    if n > 1:
        assert np.array_equal(ban_spec.ngram_banned(first, n), [first[n - 1]])
        assert np.array_equal(ban_spec.ngram_banned(last, n), [last[L - 1]])


def test_ban_kernel_overwrites_and_static_alone():
    """Two calls on the same buffer with different histories: the second result holds nothing of the first.  n = 0: the
    static list (and eos) alone, whatever the histories say."""
    V = 1025
    rng = np.random.default_rng(9)
    a = [rng.choice([5, 6, 7, 900], 300) for _ in range(4)]
    b = [rng.choice([40, 41, 1024], 300) for _ in range(3)] + [np.zeros(0, dtype=np.int64)]
    g1, buf = _ban_kernel(a, 2, [3], V, cap=300)
    g2, _ = _ban_kernel(b, 2, [17], V, out=buf, cap=300)
    assert np.array_equal(g1, _want_words(a, 2, [3], V)) and np.array_equal(g2, _want_words(b, 2, [17], V))
    assert g1.any() and not np.array_equal(g1, g2)
    g3, _ = _ban_kernel(a, 0, br.SUPPRESS, V, eos=999, out=buf, cap=300)
    want = ban_spec.ban_words(ban_spec.banned_mask([], 0, V, dict(suppress_tokens=br.SUPPRESS, min_new_tokens=1), eos_token_id=999))
    assert np.array_equal(g3, np.tile(want, (4, 1)))


def test_ban_hook_refusals():
    lib = capi.lib()
    dh = torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, 33, dtype=torch.int32, device="cuda")
    neg = (C.c_int32 * 2)(4, -1)
    for lens, n, st, ns, word in (([3, 9], 2, None, 0, "length 9"), ([3, 3], 17, None, 0, "no_repeat_ngram_size"), ([3, 3], 2, neg, 2, "negative id")):
        dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        rc = lib.mtts_k_ngram_ban(dh.data_ptr(), dl.data_ptr(), 2, 8, n, st, ns, 1025, -1, 0, out.data_ptr(), None)
        assert rc == capi.EINVAL and word in lib.mtts_last_error().decode(), lib.mtts_last_error()


# ---- 2. the sampler with bans against HF ----------------------------------------------------------------------------------
class _Rows:
    """Logits, history bitmaps and ban words of one case on the device, uploaded once; sample() is one hook call."""

    def __init__(self, logits, hist, words, V):
        self.rows, self.V = logits.shape[0], V
        self.lt = torch.from_numpy(np.array(logits, dtype=np.float32)).to(torch.bfloat16).cuda()
        bm = np.zeros((self.rows, (V + 31) // 32), dtype=np.uint32)
        for b in range(self.rows):
            for t in hist[b]:
                bm[b, t >> 5] |= np.uint32(1 << (t & 31))
        self.bm = torch.from_numpy(bm.view(np.int32)).cuda()
        self.ban = torch.from_numpy(np.array(words).view(np.int32)).cuda()
        self.zero = torch.zeros_like(self.ban)
        self.mask_id, self.channel = fr.VOCABS[V]["mask_id"], fr.VOCABS[V]["channel"]

    def sample(self, lc, do_sample, step, ban="case", hook="bans"):
        lib = capi.lib()
        cfg = sampler_cfgs([lc] * 8, [do_sample] * 8)[0]
        tok = torch.full((self.rows,), -7, dtype=torch.int32, device="cuda")
        lpt = torch.full((self.rows,), 7.0, dtype=torch.float32, device="cuda")
        args = (self.lt.data_ptr(), self.rows, self.V, self.bm.data_ptr(), C.byref(cfg), self.mask_id, C.c_uint64(fr.SEED), step,
                self.channel, tok.data_ptr(), lpt.data_ptr())
        if hook == "scores":
            capi.check(lib.mtts_k_sample_scores(*args, None))
        else:
            arr = sampler_floors([lc] * 8, [do_sample] * 8)
            fl = None if arr is None else C.byref(arr[0])
            bp = {"case": self.ban, "zero": self.zero, None: None}[ban]
            capi.check(lib.mtts_k_sample_bans(*args, fl, None if bp is None else bp.data_ptr(), None))
        torch.cuda.synchronize()
        return tok.cpu().numpy().astype(np.int64), lpt.cpu().numpy()


@pytest.mark.parametrize("mode", list(br.MODES))
@pytest.mark.parametrize("V", list(br.VOCABS))
def test_sampler_with_bans_vs_hf(V, mode):
    """6 rows x 6 steps per case, the shape of test_kernel_vs_hf_warpers, with HF's chain RepetitionPenalty -> NoRepeatNGram
    -> SuppressTokens -> Temperature -> TopK -> TopP (-> MinP).  The pick is the token oracle.sample_from_scores draws from
    HF's row (a greedy channel: its argmax); lp is within 2e-5 of the float64 log-softmax of that row.  Where top-p acts on
    the full-vocabulary path the mass allowance of that test applies (1e-4 of mass for the pick, 1e-4 / top_p more for lp)."""
    lc, ds = br.MODES[mode]
    logits, hist, words, want = br.case(V, mode)
    banned = np.stack([ban_spec.banned_mask(h, 0, V, lc) for h in hist])
    # the bans bite: the n-gram rule removes one of the row's 12 most probable tokens, the list at least three more
    assert (banned.sum(-1) >= 4).all() and np.isinf(want[banned]).all() and all(banned[b, hist[b, 1]] for b in range(br.ROWS))
    dev = _Rows(logits, hist, words, V)
    nucleus_full = bool(ds and fr.full_path(V, lc) and lc.get("top_p"))
    tol = TOL + (1e-4 / lc["top_p"] if nucleus_full else 0.0)
    worst = 0.0
    for step in range(br.STEPS):
        tok, lp = dev.sample(lc, ds, step)
        tok2, lp2 = dev.sample(lc, ds, step)
        assert np.array_equal(tok, tok2) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32))
        draw = ao.sample_from_scores(want, fr.SEED, step, dev.channel) if ds else np.argmax(want, -1)
        for b in range(br.ROWS):
            assert 0 <= tok[b] < V and np.isfinite(want[b, tok[b]]) and not banned[b, tok[b]], (mode, V, step, b, int(tok[b]))
            if nucleus_full:
                kept = np.nonzero(np.isfinite(want[b]))[0]
                kept = kept[np.lexsort((kept, want[b][kept]))[::-1]]
                e = np.exp((want[b][kept] - want[b][kept].max()).astype(np.float32)).astype(np.float64)
                cum = np.cumsum(e) / e.sum()
                u = float(ao.philox_uniform(fr.SEED, step, b, dev.channel))
                j = int(np.nonzero(kept == tok[b])[0][0])
                lo = cum[j - 1] if j else 0.0
                assert lo - 1e-4 <= u <= cum[j] + 1e-4, (mode, V, step, b, lo, u, cum[j])
            else:
                assert tok[b] == draw[b], (mode, V, step, b, int(tok[b]), int(draw[b]))
            ref = sr.log_softmax64(want[b], tok[b])
            worst = max(worst, abs(float(lp[b]) - ref))
            assert abs(float(lp[b]) - ref) <= tol, (mode, V, step, b, float(lp[b]), ref, tol)
    print(f"bans {mode} V={V}: banned {banned.sum(-1).tolist()}, max |lp - fp64| = {worst:.3e} (tolerance {tol:.3e})")


@pytest.mark.parametrize("V", list(br.VOCABS))
def test_no_bans_is_the_plain_sampler_bit_for_bit(V):
    """Ban pointer NULL or all-zero words: tokens and lp are those of mtts_k_sample_scores, sampled (in-block and
    full-vocabulary) and greedy."""
    logits, hist, words, _ = br.case(V, "top_k_top_p")
    dev = _Rows(logits, hist, words, V)
    for lc, ds in ((dict(repetition_penalty=1.1, temperature=0.9, top_k=50, top_p=0.9), True),
                   (dict(repetition_penalty=1.2, temperature=1.3), True), (dict(repetition_penalty=1.2), False)):
        for step in range(2):
            tok, lp = dev.sample(lc, ds, step, hook="scores")
            for ban in (None, "zero"):
                t2, l2 = dev.sample(lc, ds, step, ban=ban)
                assert np.array_equal(tok, t2) and np.array_equal(lp.view(np.uint32), l2.view(np.uint32)), (V, ban, step, ds)


@pytest.mark.parametrize("V", list(br.VOCABS))
def test_every_token_banned_gives_token_0_and_nan(V):
    """All-ones ban words: token 0 with lp NaN, greedy and sampled, with and without top_k (on 152 697 tokens: the candidate
    path and the full-vocabulary kernel)."""
    logits, hist, words, _ = br.case(V, "top_k_top_p")
    dev = _Rows(logits, hist, np.full_like(np.array(words), 0xFFFFFFFF), V)
    for lc, ds in ((dict(temperature=0.9, top_k=50, top_p=0.9), True), (dict(repetition_penalty=1.1, temperature=1.1, top_p=0.9), True),
                   (dict(temperature=0.9), True), (dict(repetition_penalty=1.1), False)):
        tok, lp = dev.sample(lc, ds, 1)
        assert np.array_equal(tok, np.zeros(br.ROWS, dtype=np.int64)) and np.isnan(lp).all(), (V, lc, ds, tok, lp)
    # the scratch the all-banned rows went through is clean: the next call is a fresh one
    logits, hist, words, _ = br.case(V, "top_p")
    lc, ds = br.MODES["top_p"]
    a = _Rows(logits, hist, words, V).sample(lc, ds, 0)
    assert np.isfinite(a[1]).all()


# ---- 3. the engine, step by step ----------------------------------------------------------------------------------------------
BAN_LAYERS = ([dict(no_repeat_ngram_size=3, suppress_tokens=br.SUPPRESS)] + [dict(no_repeat_ngram_size=2, suppress_tokens=br.SUPPRESS)] * 7,
              [False] * 8)


# test_scores_gpu.py's tiny scenario with channel 0 held inside the speech range (speech rows boosted, EOS not): a greedy
# channel 0 that the trigram ban pushes off its loop then lands on another speech token instead of ending the dialogue
BAN_SCENARIO = dict(sr.SCENARIO, wkw=dict(emb_row_sigma=0.6, speech_boost=8.0, eos_boost=1.0))


def _scenario(dtype, sc=sr.SCENARIO):
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, sc["weight_seed"], bf16=(dtype == "bf16"), **sc["wkw"])
    ids, mask = synth.synth_prompts(cfg, sc["prompt_seed"], sc["batch"], sc["prompt_len"], sc["audio_frac"], True)
    return sc, cfg, w, ids, mask


def _engine(cfg, w, dtype="bf16", max_batch=4):
    eng = Engine(cfg, max_batch=max_batch, max_seq_len=256, dtype=dtype)
    eng.bind_state_dict(w)
    return eng


def _stepped_run(eng, ids, mask, ml, layers, ds, seed, new, keep_logits=False, takes=1):
    eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=seed, takes=takes)
    plan = eng.step_plan(1)
    logs = []
    for _ in range(new + 8):
        if keep_logits:
            logs.append(eng.read_logits())
        eng.step(1)
        if eng.sync_state()[1]:
            break
    return eng.read_generated(new + 16), logs, plan


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_engine_greedy_steps_are_hf_argmax(dtype):
    """Ragged left-padded B=3, greedy, about 40 steps, no_repeat_ngram_size 3 on channel 0 and 2 on the speech channels plus
    the suppress list.  Per step read_logits() then step(1): every appended model decision is the argmax (lowest id among
    equals) of HF's processors applied to those logits and the history so far (padded prompt slots included).  The ban must
    have displaced the unbanned argmax in at least 8 decisions."""
    sc, cfg, w, ids, mask = _scenario(dtype, BAN_SCENARIO)
    layers, ds = BAN_LAYERS
    new = 40
    ml = ids.shape[1] + new
    base = ids.shape[1] - 7
    assert (mask[:, :base] == 0).any()                                   # a left-padded row: its padding is history
    eng = _engine(cfg, w, dtype)
    gen, logs, plan = _stepped_run(eng, ids, mask, ml, layers, ds, 0, new, keep_logits=True)
    assert any(line.startswith("sample:") and "bans" in line.split() for line in plan), plan
    G = gen.shape[0]
    used = sr.used_mask(gen, base, ml, cfg)
    displaced = checked = 0
    for g in range(G):
        l0, l17 = logs[g]
        for r in range(ids.shape[0]):
            for c in range(8):
                if not used[g, r, c]:
                    continue
                row = l0[r] if c == 0 else l17[c - 1, r]
                history = np.concatenate([ids[r, :base, c], gen[:g, r, c]])
                s = br.hf_step_row(row, history, layers[c], g, c, cfg["eos_token_id"], base)
                assert int(gen[g, r, c]) == int(np.argmax(s)), (dtype, g, r, c, int(gen[g, r, c]), int(np.argmax(s)))
                checked += 1
                displaced += int(np.argmax(sr.masked(row, g, c)) != np.argmax(s))
    print(f"engine bans {dtype}: {checked} decisions, the ban displaced the unbanned argmax in {displaced}")
    assert G >= 35 and displaced >= 8, (G, checked, displaced)
    eng.close()


# ---- 4. the same tokens across run modes ----------------------------------------------------------------------------------------
SAMPLED_BANS = ([dict(lc, no_repeat_ngram_size=3 if i == 0 else 2, suppress_tokens=br.SUPPRESS) for i, lc in enumerate(sr.SCENARIO_SAMPLED[0])],
                sr.SCENARIO_SAMPLED[1])


def test_graph_replay_and_plain_launches_agree(monkeypatch):
    sc, cfg, w, ids, mask = _scenario("bf16")
    layers, ds = SAMPLED_BANS
    ml = ids.shape[1] + 24
    eng = _engine(cfg, w)
    want = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=11)
    plain = eng.generate(ids, mask, ml, layers=[fr.four(lc) for lc in layers], do_samples=ds, seed=11)
    eng.close()
    assert not _eq(want, plain)                                          # (the bans changed the run)
    monkeypatch.setenv("MTTS_GRAPHS", "0")
    eng = _engine(cfg, w)
    got = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=11)
    eng.close()
    assert _eq(got, want)


def test_static_row_scheduler_slot_eviction_and_takes():
    """Row 0 (no padding) alone: batch 1, a scheduler slot, and a slot that was evicted after 9 steps and submitted again give
    the same tokens.  num_return_sequences = 3 equals the repeat-interleaved batch, and its takes differ: each bans from its
    own history behind the shared prompt -- statically, and forked in the scheduler."""
    from mtts.scheduler import ContinuousBatcher
    sc, cfg, w, ids, mask = _scenario("bf16")
    layers, ds = SAMPLED_BANS
    new = 24
    T = ids.shape[1]
    base = T - 7
    assert mask[0].all()
    eng = _engine(cfg, w, max_batch=12)
    one = eng.generate(ids[:1], mask[:1], T + new, layers=layers, do_samples=ds, seed=11)[0]
    cb = ContinuousBatcher(eng, slots=2, gen_cap=new + 16, layers=layers, do_samples=ds)
    assert any("bans" in line for line in eng.step_plan(1))
    res = cb.run([ids[0]], new, seeds=[11], row_ids=[0])
    assert _eq(res[0], one[:res[0].shape[0]]) and res[0].shape[0] - base >= 8
    # eviction after 9 steps, another dialogue through the slot's history row, then the first one again
    eng.sched_open(2, new + 16, layers=layers, do_samples=ds)
    eng.submit(0, ids[0], T + new, seed=11, row_id=0)
    eng.step(9)
    eng.evict(0)
    other = np.ascontiguousarray(ids[2][int(np.argmax(mask[2] > 0)):])     # (row 2 without its left padding)
    eng.submit(0, other, other.shape[0] + 6, seed=5, row_id=0)
    eng.step(4)
    eng.evict(0)
    eng.submit(0, ids[0], T + new, seed=11, row_id=0)
    for _ in range(new + 16):
        eng.step(1)
        if not eng.slot_states()[0, 0]:
            break
    again = eng.slot_read(0, new + 16)
    assert _eq(again, res[0][base:])
    # takes
    rep = np.repeat(ids, 3, axis=0), np.repeat(mask, 3, axis=0)
    a = eng.generate(ids, mask, T + new, layers=layers, do_samples=ds, seed=11, takes=3)
    b = eng.generate(rep[0], rep[1], T + new, layers=layers, do_samples=ds, seed=11)
    assert _eq(a, b) and not _eq(a[0], a[1]) and not _eq(a[1], a[2])
    cb = ContinuousBatcher(eng, slots=4, gen_cap=new + 16, layers=layers, do_samples=ds)
    res = cb.run([ids[0]], new, seeds=[11], row_ids=[0], takes=3)
    assert cb.forks == 2
    for j in range(3):
        assert _eq(res[j], a[j][:res[j].shape[0]]), j
    eng.close()


def test_min_new_tokens_keeps_eos_out():
    """A greedy run whose channel-0 decision of step 9 is made the model's eos_token_id: without bans the run emits EOS
    inside steps 0..9; with min_new_tokens = 5 (eos banned while step < 12) no channel-0 decision of steps 0..11 is EOS."""
    sc, cfg, w, ids, mask = _scenario("bf16")
    T = ids.shape[1]
    eng = _engine(cfg, w)
    free = eng.generate(ids[:1], mask[:1], T + 16, seed=0)[0][T - 7:]
    eng.close()
    # the token of step 9 as eos: the unbanned run then emits EOS where that token first appears, at or before step 9
    step = int(np.argmax(free[:, 0] == free[9, 0]))
    cfg2 = dict(cfg, eos_token_id=int(free[9, 0]))
    eng = _engine(cfg2, w)
    plain = eng.generate(ids[:1], mask[:1], T + 16, seed=0)[0][T - 7:]
    assert plain[step, 0] == cfg2["eos_token_id"] and _eq(plain[:step + 1], free[:step + 1])
    kept = eng.generate(ids[:1], mask[:1], T + 16, layers=[dict(min_new_tokens=5)] * 8, seed=0)[0][T - 7:]
    dec = sr.used_mask(kept[:, None, :], T - 7, T + 16, cfg2)[:, 0, 0]       # (a flush appends EOS on channel 0: those are no decisions)
    assert kept.shape[0] >= 12 and dec[:step + 1].all() and _eq(kept[:step], plain[:step])
    assert not (kept[:12, 0][dec[:12]] == cfg2["eos_token_id"]).any()
    eng.close()


# ---- 5. the off path ------------------------------------------------------------------------------------------------------------
def test_a_run_without_bans_launches_and_allocates_what_it_did():
    sc, cfg, w, ids, mask = _scenario("bf16")
    layers, ds = sr.SCENARIO_SAMPLED
    ml = ids.shape[1] + 12
    lib = capi.lib()
    free0 = torch.cuda.mem_get_info()[0]
    eng = _engine(cfg, w)
    n0 = lib.mtts_debug_ban_launches()
    eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=3)
    plan = eng.step_plan(1)
    assert not any("bans" in line for line in plan)
    sample = [line for line in plan if line.startswith("sample:")]
    assert sample == ["sample: ch0_sampled topk=0"], sample              # the text a run without bans has always had
    eng.step(6)
    eng.sync_state()
    assert lib.mtts_debug_ban_launches() == n0
    used_plain = free0 - torch.cuda.mem_get_info()[0]
    # an all-absent table is no table
    eng.begin(ids, mask, ml, layers=[dict(lc, no_repeat_ngram_size=0, suppress_tokens=[], min_new_tokens=0) for lc in layers], do_samples=ds, seed=3)
    eng.step(2)
    eng.sync_state()
    assert lib.mtts_debug_ban_launches() == n0 and free0 - torch.cuda.mem_get_info()[0] == used_plain
    # static bans: the ban words, no history; an n-gram ban: the history too
    eng.begin(ids, mask, ml, layers=[dict(lc, suppress_tokens=[5]) for lc in layers], do_samples=ds, seed=3)
    eng.step(2)
    eng.sync_state()
    used_static = free0 - torch.cuda.mem_get_info()[0]
    assert lib.mtts_debug_ban_launches() > n0 and used_static >= used_plain
    eng.begin(ids, mask, ml, layers=[dict(lc, no_repeat_ngram_size=2) for lc in layers], do_samples=ds, seed=3)
    eng.step(2)
    eng.sync_state()
    assert free0 - torch.cuda.mem_get_info()[0] >= used_static
    # and the run after it is a plain one again (one-shot)
    n1 = lib.mtts_debug_ban_launches()
    want = _engine(cfg, w)
    a = want.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=3)
    want.close()
    b = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=3)
    assert _eq(a, b) and lib.mtts_debug_ban_launches() == n1
    eng.close()
