"""Sampled takes per prompt (HF num_return_sequences) on shared KV pages.  -m gpu.

`Engine.generate(ids, mask, ..., takes=n)` prefills each prompt once; the n takes of prompt b (rows b*n+j) share its
complete prompt pages and copy its partially filled last page (csrc/layer.hip: fork_kernel).  Every result must equal,
bit for bit, the run of the repeat-interleaved batch, which prefills and stores every row on its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402

SAMPLED = ([dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.2)] * 8, [True] * 8)
MIXED = ([dict(repetition_penalty=1.2)] + [dict(top_k=30, top_p=0.85, temperature=1.0, repetition_penalty=1.1)] * 7,
         [False] + [True] * 7)
LENS = (128, 129, 200)          # real prompt tokens: ends on a page boundary, one token into a page, mid-page after 3 pages


def _weights(cfg, seed=301):
    return synth.synth_weights(cfg, seed, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)


def _prompts(cfg, lens, seed):
    """Left-padded batch whose row b holds exactly lens[b] real tokens (half text, half audio), delay-shifted."""
    rng = np.random.default_rng(seed)
    seqs = []
    for n in lens:
        raw = np.full((n, 8), 1024, dtype=np.int64)
        na = n // 2
        raw[:n - na, 0] = rng.integers(0, 151643, n - na)
        raw[n - na:, 0] = 151665 + rng.integers(0, 1024, na)
        raw[n - na:, 1:] = rng.integers(0, 1024, (na, 7))
        seqs.append(synth.shifting_inputs(raw, cfg["pad_token_id"]))
    return synth.left_pad(seqs, cfg["pad_token_id"])


def _engine(cfg, w, **kw):
    from mtts.engine import Engine
    kw.setdefault("max_batch", 12)
    kw.setdefault("max_seq_len", 512)
    eng = Engine(cfg, **kw)
    eng.bind_state_dict(w)
    return eng


def _pages(lens, n):
    """Pages a forked begin takes: every prompt's pages once, plus one private copy of each partial last page per take."""
    return sum(-(-L // 64) for L in lens) + (n - 1) * sum(1 for L in lens if L % 64)


def _check_tables(eng, lens, n, max_batch=12):
    """Right after begin(takes=n): the pool's free count, the device table, and the sharing pattern."""
    total, free, _ = eng.kv_pool_state()
    assert free == total - _pages(lens, n)
    host, npg = eng.page_table(max_batch)
    dev = eng.device_page_table(max_batch)
    owned = []
    for b, L in enumerate(lens):
        rows = list(range(b * n, (b + 1) * n))
        full = L // 64
        src = host[rows[0], :npg[rows[0]]]
        mine = set(src.tolist())
        for r in rows:
            assert npg[r] == -(-L // 64)
            assert np.array_equal(host[r, :npg[r]], dev[r, :npg[r]]), r
            assert np.array_equal(host[r, :full], src[:full]), r          # the complete pages are shared ...
            private = host[r, full:npg[r]].tolist()
            if r != rows[0]:
                assert not set(private) & set(src.tolist()), r           # ... and nothing else
            mine |= set(private)
        owned.append(mine)
    for b1 in range(len(lens)):
        for b2 in range(b1 + 1, len(lens)):
            assert not owned[b1] & owned[b2], (b1, b2)                     # no page in two prompts' tables
    assert total - free == len(set().union(*owned))                       # and no page handed out twice


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("mode", ["sealed", "bf16_pages", "shuffled"])
def test_takes_equal_repeat_interleaved_batch(monkeypatch, mode):
    """3 prompts x 4 takes, all channels sampled (repetition penalty, top-k, top-p) and greedy channel 0 + sampled speech
    channels.  max_length lets every row cross 2+ page boundaries after the fork and cuts rows off, so the static batch's
    flush / resurrection semantics are part of the comparison.  Logits after `begin` are compared bit for bit too."""
    if mode == "bf16_pages":
        monkeypatch.setenv("MTTS_KV_PACK", "0")
    if mode == "shuffled":
        monkeypatch.setenv("MTTS_PAGE_SHUFFLE", "17")
    cfg = synth.tiny()
    eng = _engine(cfg, _weights(cfg))
    ids, mask = _prompts(cfg, LENS, 31)
    n = 4
    base = ids.shape[1] - 7
    ml = base + 140
    ex_ids, ex_mask = np.repeat(ids, n, 0), np.repeat(mask, n, 0)
    for layers, ds in (SAMPLED, MIXED):
        got = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=99, takes=n)
        want = eng.generate(ex_ids, ex_mask, ml, layers=layers, do_samples=ds, seed=99)
        assert got.shape == want.shape == (len(LENS) * n, got.shape[1], 8)
        assert np.array_equal(got, want)
        assert got.shape[1] - base >= 140                                    # rows ran into max_length
        for b in range(len(LENS)):
            takes = got[b * n:(b + 1) * n, base:]
            assert any(not np.array_equal(takes[0], takes[j]) for j in range(1, n)), "takes of one prompt are identical"
        eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=99, takes=n)
        g0, g17 = eng.read_logits()
        eng.begin(ex_ids, ex_mask, ml, layers=layers, do_samples=ds, seed=99)
        w0, w17 = eng.read_logits()
        assert np.array_equal(_bits(g0), _bits(w0)) and np.array_equal(_bits(g17), _bits(w17))
    eng.close()


def test_takes_share_complete_prompt_pages():
    cfg = synth.tiny()
    eng = _engine(cfg, _weights(cfg), max_batch=12)
    ids, mask = _prompts(cfg, LENS, 32)
    eng.begin(ids, mask, ids.shape[1] - 7 + 40, *SAMPLED, seed=3, takes=4)
    _check_tables(eng, LENS, 4)
    eng.close()


def test_takes_plain_takes_on_one_engine_no_leak():
    """Takes, then a plain batch, then takes again on one engine: each run equals the same run on a fresh engine, every
    page comes back after a run, and the next begin takes exactly what its prompts need (a page freed twice would be
    handed to two rows: the plain run's tables must be disjoint)."""
    cfg = synth.tiny()
    w = _weights(cfg, 302)
    eng = _engine(cfg, w)
    ids, mask = _prompts(cfg, LENS, 33)
    ml = ids.shape[1] - 7 + 90
    total = eng.kv_pool_state()[0]
    assert total == 12 * 9
    for k, n in enumerate((4, 1, 3)):
        fresh = _engine(cfg, w)
        got = eng.generate(ids, mask, ml, *SAMPLED, seed=40 + k, takes=n)
        assert np.array_equal(got, fresh.generate(ids, mask, ml, *SAMPLED, seed=40 + k, takes=n)), n
        fresh.close()
        # rows cut off at max_length keep their pages until the next begin, which returns every page of the run
        eng.begin(ids, mask, ml, *SAMPLED, seed=1, takes=n)
        _check_tables(eng, LENS, n)
    eng.begin(ids[:1], mask[:1], ml, *SAMPLED, seed=1)
    assert eng.kv_pool_state()[1] == total - _pages(LENS[:1], 1)
    eng.close()


def test_takes_fit_where_the_expanded_batch_does_not():
    cfg = synth.tiny()
    w = _weights(cfg, 303)
    ids, mask = _prompts(cfg, LENS, 34)
    n = 4
    ml = ids.shape[1] - 7 + 16
    ex_ids, ex_mask = np.repeat(ids, n, 0), np.repeat(mask, n, 0)
    pool = 35                                   # the expanded prompts need 36 pages, the forked ones 15
    assert _pages(LENS, n) < pool < _pages(LENS, 1) * n
    small = _engine(cfg, w, kv_pool_pages=pool)
    with pytest.raises(capi.MttsError) as ei:
        small.begin(ex_ids, ex_mask, ml, *SAMPLED, seed=8)
    assert ei.value.code == capi.ENOMEM
    got = small.generate(ids, mask, ml, *SAMPLED, seed=8, takes=n)
    big = _engine(cfg, w)
    assert np.array_equal(got, big.generate(ex_ids, ex_mask, ml, *SAMPLED, seed=8))
    small.close()
    big.close()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_takes_fp32_engines(dtype):
    cfg = synth.tiny()
    eng = _engine(cfg, _weights(cfg, 304), dtype=dtype)
    ids, mask = _prompts(cfg, LENS, 35)
    n = 2
    ml = ids.shape[1] - 7 + 100
    ex_ids, ex_mask = np.repeat(ids, n, 0), np.repeat(mask, n, 0)
    for layers, ds in (SAMPLED, MIXED):
        got = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=12, takes=n)
        assert np.array_equal(got, eng.generate(ex_ids, ex_mask, ml, layers=layers, do_samples=ds, seed=12))
        eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=12, takes=n)
        g0, g17 = eng.read_logits()
        eng.begin(ex_ids, ex_mask, ml, layers=layers, do_samples=ds, seed=12)
        w0, w17 = eng.read_logits()
        assert np.array_equal(_bits(g0), _bits(w0)) and np.array_equal(_bits(g17), _bits(w17))
    eng.close()


def _plain_prompt(rng, n):
    raw = np.full((n, 8), 1024, dtype=np.int64)
    raw[:, 0] = rng.integers(0, 151643, n)
    raw[n - 6:, 0] = 151665 + rng.integers(0, 1024, 6)
    raw[n - 6:, 1:] = rng.integers(0, 1024, (6, 7))
    return synth.shifting_inputs(raw, 151643)


def test_scheduler_takes_equal_expanded_submissions():
    """5 prompts x 3 takes through 4 slots on 13 pages: takes are forked at admission, the pool runs dry mid-flight and
    dialogues are evicted and re-run as plain submissions; the result equals the batcher on the expanded prompt list."""
    from mtts.scheduler import ContinuousBatcher
    cfg = synth.tiny()
    eng = _engine(cfg, synth.synth_weights(cfg, 305, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0), max_batch=4,
                  max_seq_len=384, kv_pool_pages=13)
    rng = np.random.default_rng(12)
    prompts = [_plain_prompt(rng, int(rng.integers(70, 120))) for _ in range(5)]
    mnts = [int(rng.integers(200, 240)) for _ in range(5)]
    seeds = list(range(700, 705))
    rows = [3, 1, 4, 1, 5]
    n = 3
    cb = ContinuousBatcher(eng, slots=4, gen_cap=260, layers=SAMPLED[0], do_samples=SAMPLED[1], steps_per_poll=8)
    got = cb.run(prompts, mnts, seeds=seeds, row_ids=rows, takes=n)
    assert cb.forks > 0 and cb.evictions > 0, (cb.forks, cb.evictions)
    assert eng.kv_pool_state()[1] == 13
    ex = ContinuousBatcher(eng, slots=4, gen_cap=260, layers=SAMPLED[0], do_samples=SAMPLED[1], steps_per_poll=8)
    want = ex.run([p for p in prompts for _ in range(n)], [m for m in mnts for _ in range(n)],
                  seeds=[s for s in seeds for _ in range(n)], row_ids=[r * n + j for r in rows for j in range(n)])
    assert len(got) == len(want) == 5 * n
    for k in range(5 * n):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    eng.close()


def test_slot_fork_refuses_stepped_source_and_occupied_destination():
    cfg = synth.tiny()
    eng = _engine(cfg, _weights(cfg, 306), max_batch=4, max_seq_len=384)
    eng.sched_open(4, 128, *SAMPLED)
    rng = np.random.default_rng(4)
    p, q = _plain_prompt(rng, 90), _plain_prompt(rng, 40)
    eng.submit(0, p, p.shape[0] + 60, seed=1, row_id=0)
    eng.submit(1, q, q.shape[0] + 60, seed=2, row_id=0)
    with pytest.raises(capi.MttsError) as ei:
        eng.fork(0, 1, seed=1, row_id=1)                                   # occupied destination
    assert ei.value.code == capi.ESTATE
    free = eng.kv_pool_state()[1]
    eng.fork(0, 2, seed=1, row_id=1)
    assert eng.kv_pool_state()[1] == free - 1                              # 90 tokens: one page shared, one copied
    host, npg = eng.page_table(4)
    assert npg[2] == 2 and host[2, 0] == host[0, 0] and host[2, 1] != host[0, 1]
    eng.step(1)
    with pytest.raises(capi.MttsError) as ei:
        eng.fork(0, 3, seed=1, row_id=2)                                   # the source has stepped
    assert ei.value.code == capi.ESTATE
    eng.close()


def test_dropin_num_return_sequences():
    from modeling_asteroid import AsteroidTTSInstruct, GenerationConfig
    cfg = synth.tiny()
    w = {k: torch.from_numpy(v) for k, v in _weights(cfg, 307).items()}
    gc = GenerationConfig(do_sample=True, top_k=30, top_p=0.9, temperature=1.0, repetition_penalty=1.1,
                          eos_token_id=cfg["eos_token_id"])
    m = AsteroidTTSInstruct.from_state_dict(cfg, w, gc).to("cuda")
    ids, mask = synth.synth_prompts(cfg, 41, 3, 90, 0.4, True)
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    got = m.generate(ids, mask, max_new_tokens=48, num_return_sequences=3, seed=5)
    want = m.generate(ids.repeat_interleave(3, 0), mask.repeat_interleave(3, 0), max_new_tokens=48, seed=5)
    assert got.shape[0] == 9 and torch.equal(got, want)
    # a sharded rank's rows keep their job-wide Philox ids: take j of row r draws as row r*n+j
    m.sample_rows = [5, 9]
    got = m.generate(ids[:2], mask[:2], max_new_tokens=48, num_return_sequences=2, seed=6)
    m.sample_rows = [10, 11, 18, 19]
    want = m.generate(ids[:2].repeat_interleave(2, 0), mask[:2].repeat_interleave(2, 0), max_new_tokens=48, seed=6)
    m.sample_rows = None
    assert torch.equal(got, want)
    # n = 1 is the call without the keyword
    assert torch.equal(m.generate(ids, mask, max_new_tokens=32, num_return_sequences=1, seed=7),
                       m.generate(ids, mask, max_new_tokens=32, seed=7))
    # more rows than one engine pass: the scheduled path, with takes
    big_ids, big_mask = synth.synth_prompts(cfg, 42, 44, 40, 0.4, True)
    big_ids, big_mask = torch.from_numpy(big_ids), torch.from_numpy(big_mask)
    got = m.generate(big_ids, big_mask, max_new_tokens=24, num_return_sequences=3, seed=9)
    want = m.generate(big_ids.repeat_interleave(3, 0), big_mask.repeat_interleave(3, 0), max_new_tokens=24, seed=9)
    assert got.shape[0] == 132 and torch.equal(got, want)
