"""Sequence rules and step-conditioned bans (sequence_bias, bad_words_ids, min_length, begin_suppress_tokens) on the device.
-m gpu.

The reference is HF itself (tests/bias_ref.py: the installed transformers' processors on CPU torch) and mtts/bias_spec.py,
which tests/test_sampler_bias_cpu.py holds against them.  The rule kernel is held against bias_spec exactly.  The sampler adds
one fp32 addition per biased token, the one HF makes, so its scores are HF's on the bits; lp is held to 1e-6 against the
float64 log-softmax of HF's row, and each row prints the kernel's lp beside HF's own fp32 log-softmax and the float64 value.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import ban_spec, bias_spec, capi, synth  # noqa: E402
from mtts.engine import Engine, sampler_bias, sampler_cfgs, sampler_floors  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import bias_ref as bf  # noqa: E402
import floors_ref as fr  # noqa: E402
import scores_ref as sr  # noqa: E402

LP_TOL = 1e-6


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- 1. the rule kernel against bias_spec, exact --------------------------------------------------------------------------
class _Kernel:
    """mtts_k_seq_bias on a list of histories; the output buffers are kept so that a second call finds them stale."""

    def __init__(self, rows, V, ban_fill=0):
        words = (V + 31) // 32
        self.V, self.rows = V, rows
        self.ban0 = torch.full((rows, words), ban_fill, dtype=torch.int32, device="cuda")
        self.bw = torch.full((rows, words), -1, dtype=torch.int32, device="cuda")      # (stale bits everywhere: the kernel overwrites)
        self.tab = torch.full((rows, C.sizeof(capi.MttsBiasTable) // 4), 0x7fc00001, dtype=torch.int32, device="cuda")

    def run(self, hists, layer, cap=None):
        cap = max([len(h) for h in hists] + [1]) if cap is None else cap
        hm = np.full((self.rows, cap), -3, dtype=np.int32)
        for r, h in enumerate(hists):
            hm[r, :len(h)] = h
        dh = torch.from_numpy(hm).cuda()
        dl = torch.tensor([len(h) for h in hists], dtype=torch.int32, device="cuda")
        ban = self.ban0.clone()
        arr = sampler_bias([layer] * 8)
        capi.check(capi.lib().mtts_k_seq_bias(dh.data_ptr(), dl.data_ptr(), self.rows, cap, C.byref(arr[0]), self.V, ban.data_ptr(),
                                              self.bw.data_ptr(), self.tab.data_ptr(), None))
        torch.cuda.synchronize()
        raw = self.tab.cpu().numpy()
        tabs = [(raw[r, 1:1 + raw[r, 0]].astype(np.int32), raw[r, 65:65 + raw[r, 0]].view(np.float32).copy()) for r in range(self.rows)]
        return ban.cpu().numpy().view(np.uint32), self.bw.cpu().numpy().view(np.uint32), tabs


def _want(hists, layer, V, ban0=None):
    rules, _, _ = bias_spec.bias_of(layer)
    ban, words, tabs = [], [], []
    for r, h in enumerate(hists):
        m = bias_spec.banned_mask(h, 0, V, layer)
        ban.append(ban_spec.ban_words(m) | (0 if ban0 is None else ban0[r]))
        ids, terms = bias_spec.bias_terms(h, V, rules)
        bits = np.zeros(V, dtype=bool)
        bits[ids] = True
        words.append(ban_spec.ban_words(bits))
        tabs.append((ids, terms))
    return np.stack(ban), np.stack(words), tabs


def _same(got, want, what):
    gb, gw, gt = got
    wb, ww, wt = want
    assert np.array_equal(gb, wb), (what, "ban words", np.argwhere(gb != wb)[:5])
    assert np.array_equal(gw, ww), (what, "bias words", np.argwhere(gw != ww)[:5])
    for r, ((gi, gv), (wi, wv)) in enumerate(zip(gt, wt)):
        assert np.array_equal(gi, wi) and np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), (what, "table", r, gi, wi, gv, wv)


def _rule_case(V, rng):
    """Rules of 1, 2, 3 and 16 tokens over an alphabet spread over the vocabulary (token V-1, in the tail word, among them),
    chains of up to three rules on one token, -inf rules of one and two tokens, ids beyond 1025; histories of 0..300 tokens
    whose tails complete some of the rules, one of them exactly as long as its rule."""
    alpha = np.concatenate([rng.choice(V - 1, 7, replace=False), [V - 1]]).tolist()
    a, b, c, d, e, f, g, last = alpha
    long = tuple(int(t) for t in rng.choice(alpha, 16))
    seq = {(a,): 0.1, (b,): -2.7, (last,): 0.3, (c, a): 0.2, (d, c, a): 0.7, (e, a): 1e-3, (c, b): 1.1, (c, f): -0.4,
           (d, c, last): 3.3, (c, g): float("-inf"), long: 2.2, (d, e, f, g): 5.0, (c, 1030): 0.5, (2000, a): 4.0}
    layer = dict(sequence_bias=seq, bad_words_ids=[[e], [c, last], [d, e, f, b], [7, 1030]])
    tails = [[], [c], [d, c], [e], [d, e, f], list(long[:-1]), [a, b], [d, c], list(long[:-1])]
    hists = []
    for length, tail in zip((0, 1, 2, 15, 16, 300, 40, 3, 15), tails):
        h = rng.choice(alpha, length)
        if len(tail) <= length:
            h[length - len(tail):] = tail
        hists.append(h)
    return layer, hists


@pytest.mark.parametrize("V", [1025, 152697])
def test_rule_kernel_is_bias_spec(V):
    """Ban words (ORed into what the buffer held), bias words and tables equal bias_spec exactly; the bias words and tables are
    overwritten although they start as all ones / garbage, bits at and above V stay 0 (152 697 is no multiple of 32); a
    second launch on the stale outputs of the first, with other histories, holds nothing of it; two launches on the same
    inputs give identical bits."""
    rng = np.random.default_rng(17 + V % 97)
    layer, hists = _rule_case(V, rng)
    k = _Kernel(len(hists), V)
    got = k.run(hists, layer)
    want = _want(hists, layer, V)
    _same(got, want, (V, "first"))
    assert sum(len(t[0]) for t in want[2]) > 3 * len(hists) and want[0].any() and max(len(t[0]) for t in want[2]) >= 4
    again = k.run(hists, layer)
    _same(again, got, (V, "again"))
    other = [h[::-1].copy() for h in hists[::-1]]
    _same(k.run(other, layer), _want(other, layer, V), (V, "stale"))
    # the ban words are ORed into: what ban_kernel left stays
    k2 = _Kernel(len(hists), V, ban_fill=0x00010001)
    _same(k2.run(hists, layer), _want(hists, layer, V, ban0=np.full(len(hists), 0x00010001, dtype=np.uint32)[:, None]), (V, "or"))
    # 64 rules on 64 distinct tokens behind one prefix: the whole table; a single-token rule and the 15 suffixes of the
    # history in front of one token: the longest chain a history can complete (16 additions in rule order)
    base = rng.choice(V, 3, replace=False).tolist()
    h = np.array(base * 6, dtype=np.int64)
    spread = {(base[2], int(x)): float(i) - 30.5 for i, x in enumerate(rng.choice(V, 64, replace=False))}
    chain = {(7,): 0.1}
    chain.update({tuple(int(t) for t in h[len(h) - n:]) + (7,): 0.1 * (n + 1) for n in range(1, 16)})
    for lay in (dict(sequence_bias=spread), dict(sequence_bias=chain)):
        k1 = _Kernel(2, V)
        _same(k1.run([h, h[:-1]], lay), _want([h, h[:-1]], lay, V), (V, "full table"))
    assert len(_want([h], dict(sequence_bias=spread), V)[2][0][0]) == 64
    ids, terms = _want([h], dict(sequence_bias=chain), V)[2][0]
    want16 = np.float32(0.0)
    for n in range(16):
        want16 = np.float32(want16 + np.float32(0.1 * (n + 1)))
    assert ids.tolist() == [7] and terms[0] == want16


def test_rule_hook_refusals():
    lib = capi.lib()
    dh = torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, 33, dtype=torch.int32, device="cuda")
    tab = torch.zeros(2, 129, dtype=torch.int32, device="cuda")
    dl = torch.tensor([3, 9], dtype=torch.int32, device="cuda")
    arr = sampler_bias([dict(sequence_bias={(3, 4): 1.0})] * 8)
    rc = lib.mtts_k_seq_bias(dh.data_ptr(), dl.data_ptr(), 2, 8, C.byref(arr[0]), 1025, out.data_ptr(), out.data_ptr(), tab.data_ptr(), None)
    assert rc == capi.EINVAL and "length 9" in lib.mtts_last_error().decode()
    dl = torch.tensor([3, 3], dtype=torch.int32, device="cuda")
    rc = lib.mtts_k_seq_bias(dh.data_ptr(), dl.data_ptr(), 2, 8, C.byref(arr[0]), 1025, None, None, None, None)
    assert rc == capi.EINVAL and "no bias words" in lib.mtts_last_error().decode()
    arr = sampler_bias([dict(bad_words_ids=[[3, 4]])] * 8)
    rc = lib.mtts_k_seq_bias(dh.data_ptr(), dl.data_ptr(), 2, 8, C.byref(arr[0]), 1025, None, None, None, None)
    assert rc == capi.EINVAL and "no ban words" in lib.mtts_last_error().decode()
    arr[0].rule_len[0] = 17
    rc = lib.mtts_k_seq_bias(dh.data_ptr(), dl.data_ptr(), 2, 8, C.byref(arr[0]), 1025, out.data_ptr(), None, None, None)
    assert rc == capi.EINVAL and "17 tokens" in lib.mtts_last_error().decode()


# ---- 2. the sampler with bias against HF ------------------------------------------------------------------------------------
def _tables(tabs):
    raw = np.zeros((len(tabs), C.sizeof(capi.MttsBiasTable) // 4), dtype=np.int32)
    for r, (ids, terms) in enumerate(tabs):
        raw[r, 0] = len(ids)
        raw[r, 1:1 + len(ids)] = ids
        raw[r, 65:65 + len(ids)] = np.asarray(terms, dtype=np.float32).view(np.int32)
    return raw


class _Rows:
    """Logits, history bitmaps, ban words, bias words and tables of one case on the device, uploaded once."""

    def __init__(self, logits, hist, ban, words, tabs, V):
        self.rows, self.V = logits.shape[0], V
        self.lt = torch.from_numpy(np.array(logits, dtype=np.float32)).to(torch.bfloat16).cuda()
        bm = np.zeros((self.rows, (V + 31) // 32), dtype=np.uint32)
        for b in range(self.rows):
            for t in hist[b]:
                bm[b, t >> 5] |= np.uint32(1 << (t & 31))
        self.bm = torch.from_numpy(bm.view(np.int32)).cuda()
        self.ban = torch.from_numpy(np.array(ban).view(np.int32)).cuda()
        self.bw = torch.from_numpy(np.array(words).view(np.int32)).cuda()
        self.tab = torch.from_numpy(_tables(tabs)).cuda()
        self.mask_id, self.channel = fr.VOCABS[V]["mask_id"], fr.VOCABS[V]["channel"]

    def sample(self, lc, do_sample, step, bias=True, ban=True, hook="bias"):
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
            capi.check(lib.mtts_k_sample_bias(*args, fl, self.ban.data_ptr() if ban else None, C.c_float(0.0),
                                              self.bw.data_ptr() if bias else None, self.tab.data_ptr() if bias else None, None))
        torch.cuda.synchronize()
        return tok.cpu().numpy().astype(np.int64), lpt.cpu().numpy()


@pytest.mark.parametrize("mode", list(bf.MODES))
@pytest.mark.parametrize("V", list(bf.VOCABS))
def test_sampler_with_bias_vs_hf(V, mode):
    """6 rows x 6 steps per case with HF's chain SequenceBias -> RepetitionPenalty -> NoRepeatNGram -> NoBadWords ->
    SuppressTokens -> Temperature -> TopK -> TopP (-> MinP).  The rules bite on every row (asserted below): a positive term
    makes a non-maximal token the argmax, a negative one sits on the raw maximum, a term flips the sign of a token with the
    history bit, a term sits on the masked id, a -inf rule fires.  Same kept set as HF (the pick is a member, and it is the
    token oracle.sample_from_scores draws from HF's row; a greedy channel: its argmax), lp within 1e-6 of the float64
    log-softmax of HF's row on every path.  Where top-p acts on the full-vocabulary path (about 10 000 kept tokens of 1e-5
    of mass each, where no redraw can keep HF's own fp32 cumulative sum off every boundary) the pick is held as
    test_sampler_bans_gpu.py holds it: its CDF interval in HF's row contains u within 1e-4 of mass.  Every row is compared.
    Measured on an MI355X: the largest |lp - fp64| is 3.7e-7 (top_p on 152 697 tokens); HF's own fp32 log-softmax lies up to
    6.5e-6 from the float64 value on the same rows (greedy, 152 697 tokens)."""
    lc, ds = bf.MODES[mode]
    logits, hist, ban, words, tabs, want = bf.case(V, mode)
    mask_id = fr.VOCABS[V]["mask_id"]
    pen = lc["repetition_penalty"]
    for b in range(bf.ROWS):
        assert int(np.argmax(logits[b])) == bf.DOWN and int(np.argmax(want[b])) == bf.UP          # both argmax cases
        assert np.isinf(want[b, [mask_id, bf.GONE, bf.NEXT_BAD]]).all()                             # the masked id, the -inf rules
        assert logits[b, bf.FLIP] == -0.5 and bf.FLIP in hist[b]
        assert dict(zip(*tabs[b]))[bf.UP] == np.float32(np.float32(1.7) + np.float32(0.1)) and bf.NEXT in tabs[b][0]
    # the order case, on HF's own arithmetic: (-0.5 + 1.0) / penalty, not (-0.5 * penalty) + 1.0
    flip = bf.hf_scores(logits, hist, dict(repetition_penalty=pen, sequence_bias=bf.SEQUENCE_BIAS), mask_id)[:, bf.FLIP]
    assert np.array_equal(flip, np.full(bf.ROWS, np.float32(0.5) / np.float32(pen), dtype=np.float32))
    dev = _Rows(logits, hist, ban, words, tabs, V)
    nucleus_full = bool(ds and fr.full_path(V, lc) and lc.get("top_p"))
    tol = LP_TOL
    worst = hf_gap = 0.0
    for step in range(bf.STEPS):
        tok, lp = dev.sample(lc, ds, step)
        tok2, lp2 = dev.sample(lc, ds, step)
        assert np.array_equal(tok, tok2) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32))
        draw = ao.sample_from_scores(want, fr.SEED, step, dev.channel) if ds else np.argmax(want, -1)
        for b in range(bf.ROWS):
            assert 0 <= tok[b] < V and np.isfinite(want[b, tok[b]]), (mode, V, step, b, int(tok[b]))
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
            hf32 = float(torch.log_softmax(torch.from_numpy(want[b]), -1)[tok[b]])
            hf_gap = max(hf_gap, abs(hf32 - ref))
            print(f"bias {mode} V={V} step {step} row {b}: lp {float(lp[b]):.8f} HF fp32 {hf32:.8f} fp64 {ref:.8f}")
            assert abs(float(lp[b]) - ref) <= tol, (mode, V, step, b, float(lp[b]), ref, tol)
    print(f"bias {mode} V={V}: max |lp - fp64 of HF's row| = {worst:.3e} (tolerance {tol:.3e}); HF's own fp32 is within {hf_gap:.3e}")


@pytest.mark.parametrize("V", list(bf.VOCABS))
def test_no_bias_is_the_plain_sampler_bit_for_bit(V):
    """Null bias inputs (and no ban words): tokens and lp are those of mtts_k_sample_scores, sampled (in-block and
    full-vocabulary) and greedy; with the ban words alone they are those of the bias inputs of an empty table."""
    logits, hist, ban, words, tabs, _ = bf.case(V, "top_k_top_p")
    dev = _Rows(logits, hist, ban, np.zeros_like(np.array(words)), [(np.zeros(0, np.int32), np.zeros(0, np.float32))] * bf.ROWS, V)
    for lc, ds in ((dict(repetition_penalty=1.1, temperature=0.9, top_k=50, top_p=0.9), True),
                   (dict(repetition_penalty=1.2, temperature=1.3), True), (dict(repetition_penalty=1.2), False)):
        for step in range(2):
            tok, lp = dev.sample(lc, ds, step, hook="scores")
            t2, l2 = dev.sample(lc, ds, step, bias=False, ban=False)
            assert np.array_equal(tok, t2) and np.array_equal(lp.view(np.uint32), l2.view(np.uint32)), (V, step, ds)
            t3, l3 = dev.sample(lc, ds, step, bias=False)
            t4, l4 = dev.sample(lc, ds, step, bias=True)          # all-zero bias words: no term is looked up
            assert np.array_equal(t3, t4) and np.array_equal(l3.view(np.uint32), l4.view(np.uint32)), (V, step, ds)


# ---- 3. the engine, step by step ----------------------------------------------------------------------------------------------
def _scenario(dtype, sc=sr.SCENARIO):
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, sc["weight_seed"], bf16=(dtype == "bf16"), **sc["wkw"])
    ids, mask = synth.synth_prompts(cfg, sc["prompt_seed"], sc["batch"], sc["prompt_len"], sc["audio_frac"], True)
    return sc, cfg, w, ids, mask


def _engine(cfg, w, dtype="bf16", max_batch=4):
    eng = Engine(cfg, max_batch=max_batch, max_seq_len=256, dtype=dtype)
    eng.bind_state_dict(w)
    return eng


def _stepped_run(eng, ids, mask, ml, layers, ds, seed, new):
    eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=seed)
    plan = eng.step_plan(1)
    logs = []
    for _ in range(new + 8):
        logs.append(eng.read_logits())
        eng.step(1)
        if eng.sync_state()[1]:
            break
    return eng.read_generated(new + 16), logs, plan


def _common_bigrams(gen, used, c):
    """The bigrams of channel c's decisions in a free run, most frequent first."""
    from collections import Counter
    cnt = Counter()
    for r in range(gen.shape[1]):
        col = gen[:, r, c]
        for g in range(1, gen.shape[0]):
            if used[g, r, c] and used[g - 1, r, c]:
                cnt[(int(col[g - 1]), int(col[g]))] += 1
    return [k for k, _ in cnt.most_common()]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_engine_greedy_steps_are_hf_argmax(dtype):
    """Ragged left-padded B=3, greedy, about 40 steps under the four processors on all eight channels.  The rules come from a
    free run of the same engine, so that they fire: the first model decision of a (row, channel) pair, with the token in front
    of it, becomes a 2-token bad word on two pairs and a 2-token sequence_bias of -30 on two others (channel 0 and speech
    channels: a rule of channel-0 ids is ignored on the speech channels), a frequent bigram of two more channels joins each
    list, single tokens get terms, min_length holds EOS out for 12 steps, begin_suppress_tokens names step 7's free decisions.  Per step
    read_logits() then step(1): every appended model decision is the argmax (lowest id among equals) of HF's processors
    applied to those logits and the history so far (padded prompt slots included).  Both 2-token rules must have fired, and
    the processors must have displaced the free argmax."""
    sc, cfg, w, ids, mask = _scenario(dtype)
    new = 40
    ml = ids.shape[1] + new
    base = ids.shape[1] - 7
    assert (mask[:, :base] == 0).any()                                   # a left-padded row: its padding is history
    eng = _engine(cfg, w, dtype)
    free, _, plan0 = _stepped_run(eng, ids, mask, ml, None, None, 0, new)
    assert not any("bias" in line or "rules" in line for line in plan0 if line.startswith("sample:")), plan0
    used0 = sr.used_mask(free, base, ml, cfg)


    def first(r, c):        # the first model decision of (row r, channel c) in the free run with the token in front of it
        g0 = int(np.argmax(used0[:, r, c]))
        assert used0[g0, r, c]
        return (int(free[g0 - 1, r, c]) if g0 else int(ids[r, base - 1, c]), int(free[g0, r, c]))

    # a rule on the first decision of a channel fires for certain: everything in front of it is prompt or teacher-forced
    big1, big5 = _common_bigrams(free, used0, 1), _common_bigrams(free, used0, 5)
    seq = {first(0, 0): -30.0, first(2, 5): -30.0, (int(free[20, 2, 6]),): -0.125, (152000,): 0.5}
    seq.update({b: -30.0 for b in big1[:1]})
    layer = dict(sequence_bias=seq, bad_words_ids=[list(first(1, 3)), list(first(1, 0))] + [list(b) for b in big5[:1]],
                 min_length=base + 12, begin_suppress_tokens=sorted({int(t) for t in free[7].reshape(-1)}))
    layers, ds = [layer] * 8, [False] * 8
    gen, logs, plan = _stepped_run(eng, ids, mask, ml, layers, ds, 0, new)
    assert any(line.startswith("sample:") and "bans" in line.split() and "bias" in line.split() for line in plan), plan
    G = gen.shape[0]
    used = sr.used_mask(gen, base, ml, cfg)
    fired = {"seq": 0, "bad": 0, "begin": 0}
    displaced = checked = 0
    rules, _, _ = bias_spec.bias_of(layer, eos_token_id=cfg["eos_token_id"])
    for g in range(G):
        l0, l17 = logs[g]
        for r in range(ids.shape[0]):
            for c in range(8):
                if not used[g, r, c]:
                    continue
                row = l0[r] if c == 0 else l17[c - 1, r]
                history = np.concatenate([ids[r, :base, c], gen[:g, r, c]])
                s = bf.hf_step_row(row, history, layer, g, c, cfg["eos_token_id"], base)
                assert int(gen[g, r, c]) == int(np.argmax(s)), (dtype, g, r, c, int(gen[g, r, c]), int(np.argmax(s)))
                checked += 1
                plain = sr.masked(row, g, c)
                displaced += int(np.argmax(plain) != np.argmax(s))
                tail = int(history[-1])
                fired["seq"] += int(any(len(i) == 2 and i[0] == tail and b > -np.inf and np.isfinite(plain[i[1]]) for i, b in rules if max(i) < len(s)))
                fired["bad"] += int(any(len(i) == 2 and i[0] == tail and b == -np.inf and np.isfinite(plain[i[1]]) for i, b in rules if max(i) < len(s)))
                fired["begin"] += int(g == 7)
    print(f"engine bias {dtype}: {checked} decisions, displaced {displaced}, fired {fired}")
    assert G >= 35 and fired["seq"] >= 1 and fired["bad"] >= 1 and fired["begin"] >= 1 and displaced >= 3, (G, checked, displaced, fired)
    assert not _eq(gen, free)
    eng.close()


# ---- 4. the same tokens across run modes ----------------------------------------------------------------------------------------
BIAS_KEYS = dict(sequence_bias={(3,): 0.5, (1000,): -0.75, (5000,): 1.25}, bad_words_ids=[[17], [1030]], begin_suppress_tokens=[4, 5000])


def _run_modes_layers(cfg, w, ids, mask, ml):
    """The sampled scenario's layers plus rules that fire: 2-token rules on the free run's frequent bigrams."""
    eng = _engine(cfg, w)
    layers, ds = sr.SCENARIO_SAMPLED
    free = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=11)
    eng.close()
    base = ids.shape[1] - 7
    gen = np.transpose(free[:, base:, :], (1, 0, 2))
    used = sr.used_mask(gen, base, ml, cfg)
    big0, big3 = _common_bigrams(gen, used, 0), _common_bigrams(gen, used, 3)
    seq = dict(BIAS_KEYS["sequence_bias"])
    seq.update({big0[0]: -2.5, big3[1]: 3.0})
    extra = dict(BIAS_KEYS, sequence_bias=seq, bad_words_ids=BIAS_KEYS["bad_words_ids"] + [list(big3[0])], min_length=base + 10)
    return [dict(lc, **extra) for lc in layers], ds, free


def test_graph_replay_and_plain_launches_agree(monkeypatch):
    sc, cfg, w, ids, mask = _scenario("bf16")
    ml = ids.shape[1] + 24
    layers, ds, plain = _run_modes_layers(cfg, w, ids, mask, ml)
    eng = _engine(cfg, w)
    want = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=11)
    eng.close()
    assert not _eq(want, plain)                                          # (the rules changed the run)
    monkeypatch.setenv("MTTS_GRAPHS", "0")
    eng = _engine(cfg, w)
    got = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=11)
    eng.close()
    assert _eq(got, want)


def test_static_row_scheduler_slot_eviction_and_takes():
    """Row 0 (no padding) alone: batch 1, a scheduler slot, and a slot that was evicted after 9 steps and submitted again give
    the same tokens.  num_return_sequences = 3 equals the repeat-interleaved batch, and its takes differ: each matches its
    rules against its own history behind the shared prompt -- statically, and forked in the scheduler."""
    from mtts.scheduler import ContinuousBatcher
    sc, cfg, w, ids, mask = _scenario("bf16")
    new = 24
    T = ids.shape[1]
    base = T - 7
    layers, ds, _ = _run_modes_layers(cfg, w, ids, mask, T + new)
    assert mask[0].all()
    eng = _engine(cfg, w, max_batch=12)
    one = eng.generate(ids[:1], mask[:1], T + new, layers=layers, do_samples=ds, seed=11)[0]
    cb = ContinuousBatcher(eng, slots=2, gen_cap=new + 16, layers=layers, do_samples=ds)
    assert any("bias" in line for line in eng.step_plan(1))
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


def test_min_length_keeps_eos_out():
    """A greedy run whose channel-0 decision of step 9 is made the model's eos_token_id: without the processor the run emits
    EOS at `step` <= 9.  min_length = base + 12 (eos banned while base + g < base + 12) leaves no EOS among the channel-0
    decisions of steps 0..11; min_length = base + step bans through step - 1 only, so the run is the plain one: EOS at `step`."""
    sc, cfg, w, ids, mask = _scenario("bf16")
    T = ids.shape[1]
    base = T - 7
    eng = _engine(cfg, w)
    free = eng.generate(ids[:1], mask[:1], T + 16, seed=0)[0][base:]
    eng.close()
    step = int(np.argmax(free[:, 0] == free[9, 0]))
    cfg2 = dict(cfg, eos_token_id=int(free[9, 0]))
    eng = _engine(cfg2, w)
    plain = eng.generate(ids[:1], mask[:1], T + 16, seed=0)[0][base:]
    assert plain[step, 0] == cfg2["eos_token_id"] and _eq(plain[:step + 1], free[:step + 1])
    kept = eng.generate(ids[:1], mask[:1], T + 16, layers=[dict(min_length=base + 12)] * 8, seed=0)[0][base:]
    dec = sr.used_mask(kept[:, None, :], base, T + 16, cfg2)[:, 0, 0]       # (a flush appends EOS on channel 0: those are no decisions)
    assert kept.shape[0] >= 12 and dec[:step + 1].all() and _eq(kept[:step], plain[:step])
    assert not (kept[:12, 0][dec[:12]] == cfg2["eos_token_id"]).any()
    edge = eng.generate(ids[:1], mask[:1], T + 16, layers=[dict(min_length=base + step)] * 8, seed=0)[0][base:]
    assert _eq(edge, plain)
    if step > 0:
        late = eng.generate(ids[:1], mask[:1], T + 16, layers=[dict(min_length=base + step + 1)] * 8, seed=0)[0][base:]
        assert late[step, 0] != cfg2["eos_token_id"] and _eq(late[:step], plain[:step])
    eng.close()


def test_begin_suppress_tokens_changes_exactly_one_step():
    """Greedy, stepped: with the free run's step-7 decisions as the list, every decision is the argmax of its own logits with
    the list at -inf at step 7 alone; steps 0..6 are the free run's, step 7 differs on every channel, and at no other step
    does the argmax of the unsuppressed row lose."""
    sc, cfg, w, ids, mask = _scenario("bf16")
    new = 14
    ml = ids.shape[1] + new
    base = ids.shape[1] - 7
    eng = _engine(cfg, w)
    free, _, _ = _stepped_run(eng, ids, mask, ml, None, None, 0, new)
    begin = sorted({int(t) for t in free[7].reshape(-1)})
    layer = dict(begin_suppress_tokens=begin)
    gen, logs, plan = _stepped_run(eng, ids, mask, ml, [layer] * 8, [False] * 8, 0, new)
    assert any(line.startswith("sample:") and "bans" in line.split() for line in plan), plan
    used = sr.used_mask(gen, base, ml, cfg)
    assert _eq(gen[:7], free[:7]) and gen.shape[0] >= 10
    changed = set()
    for g in range(gen.shape[0]):
        l0, l17 = logs[g]
        for r in range(ids.shape[0]):
            for c in range(8):
                if not used[g, r, c]:
                    continue
                row = sr.masked(l0[r] if c == 0 else l17[c - 1, r], g, c)
                s = bf.hf_step_row(l0[r] if c == 0 else l17[c - 1, r], np.concatenate([ids[r, :base, c], gen[:g, r, c]]), layer, g, c,
                                   cfg["eos_token_id"], base)
                assert int(gen[g, r, c]) == int(np.argmax(s)), (g, r, c)
                if int(np.argmax(s)) != int(np.argmax(row)):
                    changed.add(g)
    assert changed == {7}, changed
    assert all(int(gen[7, r, c]) not in begin for r in range(ids.shape[0]) for c in range(8) if used[7, r, c])
    eng.close()


# ---- 5. the off path ------------------------------------------------------------------------------------------------------------
def test_a_run_without_the_four_launches_and_allocates_what_it_did():
    sc, cfg, w, ids, mask = _scenario("bf16")
    layers, ds = sr.SCENARIO_SAMPLED
    ml = ids.shape[1] + 12
    lib = capi.lib()
    free0 = torch.cuda.mem_get_info()[0]
    eng = _engine(cfg, w)
    n0, b0 = lib.mtts_debug_bias_launches(), lib.mtts_debug_ban_launches()
    eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=3)
    sample = [line for line in eng.step_plan(1) if line.startswith("sample:")]
    assert sample == ["sample: ch0_sampled topk=0"], sample              # the text a run without them has always had
    eng.step(6)
    eng.sync_state()
    assert lib.mtts_debug_bias_launches() == n0 and lib.mtts_debug_ban_launches() == b0
    used_plain = free0 - torch.cuda.mem_get_info()[0]
    # an all-absent table is no table
    absent = dict(sequence_bias=None, bad_words_ids=[], min_length=0, begin_suppress_tokens=[])
    eng.begin(ids, mask, ml, layers=[dict(lc, **absent) for lc in layers], do_samples=ds, seed=3)
    eng.step(2)
    eng.sync_state()
    assert lib.mtts_debug_bias_launches() == n0 and free0 - torch.cuda.mem_get_info()[0] == used_plain
    # hard bans alone: the ban kernel, not the rule kernel
    eng.begin(ids, mask, ml, layers=[dict(lc, suppress_tokens=[5]) for lc in layers], do_samples=ds, seed=3)
    eng.step(2)
    eng.sync_state()
    assert lib.mtts_debug_bias_launches() == n0 and lib.mtts_debug_ban_launches() > b0
    # min_length alone: the ban path, no rule kernel (the step is the one captured for suppress_tokens: the counters count
    # launches by the host, a replayed step adds none); a finite single-token rule: the rule kernel, and the ban kernel rests
    eng.begin(ids, mask, ml, layers=[dict(lc, min_length=30) for lc in layers], do_samples=ds, seed=3)
    sample = [line for line in eng.step_plan(1) if line.startswith("sample:")]
    assert sample == ["sample: ch0_sampled bans topk=0"], sample
    eng.step(2)
    eng.sync_state()
    assert lib.mtts_debug_bias_launches() == n0
    b2 = lib.mtts_debug_ban_launches()
    eng.begin(ids, mask, ml, layers=[dict(lc, sequence_bias={(5,): 0.5}) for lc in layers], do_samples=ds, seed=3)
    assert any("bias" in line.split() and "bans" not in line.split() for line in eng.step_plan(1) if line.startswith("sample:"))
    eng.step(2)
    eng.sync_state()
    assert lib.mtts_debug_bias_launches() > n0 and lib.mtts_debug_ban_launches() == b2
    used_bias = free0 - torch.cuda.mem_get_info()[0]
    assert used_bias >= used_plain
    # and the run after it is a plain one again (one-shot)
    n1 = lib.mtts_debug_bias_launches()
    want = _engine(cfg, w)
    a = want.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=3)
    want.close()
    b = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=3)
    assert _eq(a, b) and lib.mtts_debug_bias_launches() == n1
    eng.close()
