"""Sequence rules and step-conditioned bans (sequence_bias, bad_words_ids, min_length, begin_suppress_tokens): the rule, the
marshalling and the host staging, on the CPU.  mtts/bias_spec.py is held against the installed transformers' own processors
(tests/bias_ref.py); tests/host/bias_stage_main.cpp runs csrc/staging.h and csrc/runstate.h under AddressSanitizer and UBSan
as a child process.  tests/test_sampler_bias_gpu.py holds the kernels and the engine against the same reference."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

from mtts import ban_spec, bias_spec, capi  # noqa: E402
from mtts.engine import sampler_bans, sampler_bias  # noqa: E402
import modeling_asteroid as ma  # noqa: E402

import bans_ref as br  # noqa: E402
import bias_ref as bf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


# ---- the rule against HF --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 152697])
def test_sequence_bias_rule_is_hfs(V):
    """Rules of 1, 2, 3 and 16 tokens over a small alphabet spread over the vocabulary, token V-1 among them, histories of
    0, 1, 2, 15, 16 and 300 tokens (shorter than a rule, one short of it, exactly it) whose tails are made to complete some of them; two and three rules ending in the same
    token (the fp32 chain, bit for bit, with betas no fp32 holds exactly); a rule ending in a token suppress_tokens bans; a
    -inf rule inside sequence_bias.  bias_row + the raw row equals HF's processor on the bits."""
    rng = np.random.default_rng(7 + V % 97)
    alpha = np.concatenate([rng.choice(V - 1, 7, replace=False), [V - 1]]).tolist()
    a, b, c, d, e, f, g, last = alpha
    long = tuple(int(t) for t in rng.choice(alpha, 16))
    sup = [t for t in br.SUPPRESS if t < V][0]
    rules = {(a,): 0.1, (b,): -2.7, (last,): 0.3, (sup,): 1.5,
             (c, a): 0.2, (d, c, a): 0.7, (e, a): 1e-3,               # a: 0.1, then + 0.2, + 0.7 where both fire
             (c, b): 1.1, (c, f): -0.4, (d, c, last): 3.3, (c, g): float("-inf"), long: 2.2, (d, e, f, g): 5.0}
    tails = [[], [c], [d, c], [e], [d, e, f], list(long[:-1]), [a, b]]
    hits = chains = 0
    for length in (0, 1, 2, 15, 16, 300):
        for tail in tails:
            h = rng.choice(alpha, length)
            if len(tail) <= length:
                h[length - len(tail):] = tail
            raw = rng.standard_normal(V).astype(np.float32) * 2.5
            raw[rng.integers(0, V)] = -np.inf
            want = bf.hf_bias(h[None], raw[None], dict(sequence_bias=rules))[0]
            row = bias_spec.bias_row(h, V, bias_spec.check_bias("sequence_bias", rules))
            got = bias_spec.apply_bias(raw, row)
            assert np.array_equal(_bits(got), _bits(want)), (V, length, tail, np.flatnonzero(_bits(got) != _bits(want))[:8])
            ids, terms = bias_spec.bias_terms(h, V, bias_spec.check_bias("sequence_bias", rules))
            assert np.array_equal(ids, np.flatnonzero((row != 0) & np.isfinite(row))) and np.array_equal(_bits(terms), _bits(row[ids]))
            hits += len(bias_spec.rule_hits(h, V, list(rules.items()))) - 4
            chains += int(row[a] not in (np.float32(0.1), np.float32(0.0)))
            if length >= 3 and tail == [d, c]:
                assert _bits(row[a]) == _bits(np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.7))) and row[g] == -np.inf
    assert hits > 10 and chains > 3
    # HF's list form and its dict: the first place, the last value
    as_list = [[[c, a], 0.5], [[a], 0.1], [[c, a], 0.2]]
    assert bias_spec.check_bias("sequence_bias", as_list) == [((c, a), 0.2), ((a,), 0.1)]


@pytest.mark.parametrize("V", [1025, 152697])
def test_bad_words_min_length_and_begin_are_hfs(V):
    """bad_words_ids with HF's EOS filter and ids on both sides of 1025 (a list with an id outside the vocabulary is ignored
    there); min_length against the width of the history; begin_suppress_tokens at exactly one step."""
    rng = np.random.default_rng(11 + V % 97)
    base, eos = 11, 999 if V == 1025 else 151643
    bad = [[eos], [5], [7, 9], [7, 1030], [1030, 9], [3, 7, 11], [2000, 4], [eos, 6]]
    layer = dict(bad_words_ids=bad)
    rules, _, _ = bias_spec.bias_of(layer, eos_token_id=eos)
    assert ((eos,), -np.inf) not in rules and ((eos, 6), -np.inf) in rules and len(rules) == len(bad) - 1
    for tail in ([], [7], [3, 7], [1030], [2000], [eos], [9]):
        h = np.concatenate([rng.integers(20, 900, 30), tail]).astype(np.int64)
        want = np.isinf(bf.hf_bias(h[None], np.zeros((1, V), dtype=np.float32), layer, eos_token_id=eos)[0])
        got = bias_spec.banned_mask(h, 0, V, layer, eos_token_id=eos)
        assert np.array_equal(got, want), (V, tail, np.flatnonzero(got != want)[:8])
        assert got[5] and not got[eos] and bool(got[9]) == (tail[-1:] == [7] or (tail == [1030] and V > 1030))
    # min_length m: eos banned while len(h) < m
    for m in (base + 3, base + 12):
        for g in (0, m - base - 1, m - base, m - base + 5):
            h = rng.integers(0, V, base + g)
            lay = dict(min_length=m, begin_suppress_tokens=[3, 1024, 1030, 152000])
            want = np.isinf(bf.hf_bias(h[None], np.zeros((1, V), dtype=np.float32), lay, step=g, eos_token_id=eos, base=base)[0])
            got = bias_spec.banned_mask(h, g, V, lay, eos_token_id=eos, base=base)
            assert np.array_equal(got, want), (V, m, g)
            assert bool(got[eos]) == (base + g < m)
    assert not bias_spec.banned_mask([], 0, 1025, dict(min_length=3), eos_token_id=151643).any()
    # begin_suppress_tokens: the one step with len(h) == base + 7
    lay = dict(begin_suppress_tokens=[3, 1024, 1030, 152000])
    fired = []
    for g in range(0, 12):
        h = rng.integers(0, V, base + g)
        want = np.isinf(bf.hf_bias(h[None], np.zeros((1, V), dtype=np.float32), lay, step=g, base=base)[0])
        got = bias_spec.banned_mask(h, g, V, lay, base=base)
        assert np.array_equal(got, want), (V, g)
        if got.any():
            fired.append(g)
            assert np.array_equal(np.flatnonzero(got), [t for t in (3, 1024, 1030, 152000) if t < V])
    assert fired == [ban_spec.DELAY_TAIL]


# ---- values and marshalling -----------------------------------------------------------------------------------------------
def test_bad_values_name_the_channel():
    many = {(i, i + 1): 0.5 for i in range(40)}
    for bad, word in ((dict(sequence_bias={(4, -1): 1.0}), "sequence_bias"), (dict(sequence_bias={(): 1.0}), "empty rule"),
                      (dict(sequence_bias={(3,): float("inf")}), "refused"), (dict(sequence_bias={(3,): float("nan")}), "refused"),
                      (dict(sequence_bias={(3,): "1"}), "number"), (dict(sequence_bias={(True,): 1.0}), "sequence_bias"),
                      (dict(sequence_bias={(2.0,): 1.0}), "sequence_bias"), (dict(sequence_bias=[[[3], 1.0, 2]]), "sequence_bias"),
                      (dict(sequence_bias=7), "sequence_bias"), (dict(sequence_bias={tuple(range(17)): 1.0}), "at most 16 tokens"),
                      (dict(bad_words_ids=[[4, -1]]), "bad_words_ids"), (dict(bad_words_ids=[[]]), "empty rule"),
                      (dict(bad_words_ids=[3]), "bad_words_ids"), (dict(bad_words_ids=[list(range(17))]), "at most 16 tokens"),
                      (dict(sequence_bias=many, bad_words_ids=[[i] for i in range(25)]), "65 rules together, at most 64"),
                      (dict(min_length=-1), "min_length"), (dict(min_length=2.0), "min_length"), (dict(min_length=True), "min_length"),
                      (dict(begin_suppress_tokens=[4, -1]), "begin_suppress_tokens"), (dict(begin_suppress_tokens=7), "begin_suppress_tokens")):
        layers = [{}] * 5 + [bad] + [{}] * 2
        with pytest.raises(ValueError, match=re.escape("layers[5]: ") + ".*" + word):
            sampler_bias(layers)
    assert bias_spec.bias_of(None) == ([], 0, []) and bias_spec.bias_of(dict(sequence_bias={}, bad_words_ids=[], min_length=0)) == ([], 0, [])
    # 64 rules of 16 tokens are taken
    full = {tuple(range(i, i + 16)): 0.5 for i in range(64)}
    assert sampler_bias([dict(sequence_bias=full)] * 8)[3].n_rules == 64


def test_marshalling():
    assert sampler_bias(None) is None and sampler_bias([{}] * 8) is None
    assert sampler_bias([dict(sequence_bias=None, bad_words_ids=[], min_length=0, begin_suppress_tokens=[], temperature=0.5)] * 8) is None
    layers = [dict(sequence_bias={(5,): 0.1, (7, 2000): -1.5}, bad_words_ids=[[9, 8, 7], [42]])] + [dict(min_length=30)] + [{}] * 5 \
        + [dict(begin_suppress_tokens=(9, 4))]
    arr = sampler_bias(layers, eos_token_id=42)
    assert [a.n_rules for a in arr] == [3, 0, 0, 0, 0, 0, 0, 0]             # ([42] is the EOS list: dropped)
    assert [a.min_length for a in arr] == [0, 30, 0, 0, 0, 0, 0, 0] and [a.n_begin_suppress for a in arr] == [0] * 7 + [2]
    assert [arr[0].rule_len[i] for i in range(3)] == [1, 2, 3] and [arr[0].rule_ids[i] for i in range(6)] == [5, 7, 2000, 9, 8, 7]
    assert _bits([arr[0].rule_bias[i] for i in range(3)]).tolist() == _bits([0.1, -1.5, -np.inf]).tolist()
    assert [arr[7].begin_suppress[i] for i in range(2)] == [9, 4]
    assert sampler_bias(layers)[0].n_rules == 4 and sampler_bans(layers) is None


def test_struct_layout_matches_the_header():
    text = open(os.path.join(ROOT, "include", "mtts.h")).read()
    body = re.search(r"typedef struct MttsSamplerBias \{(.*?)\} MttsSamplerBias;", text, re.S).group(1)
    fields = re.findall(r"^\s*(const int32_t\*|const float\*|int32_t)\s+(\w+);", body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in capi.MttsSamplerBias._fields_]
    kinds = {"int32_t": C.c_int32, "const int32_t*": C.POINTER(C.c_int32), "const float*": C.POINTER(C.c_float)}
    for (ctype, name), (_, py) in zip(fields, capi.MttsSamplerBias._fields_):
        assert py is kinds[ctype], name
    assert C.sizeof(capi.MttsSamplerBias) == 48 and capi.MttsSamplerBias.rule_len.offset == 16
    assert re.search(r"#define MTTS_BIAS_RULES_MAX (\d+)", text).group(1) == str(bias_spec.RULES_MAX)
    assert re.search(r"#define MTTS_BIAS_RULE_LEN_MAX (\d+)", text).group(1) == str(bias_spec.RULE_LEN_MAX)
    tab = re.search(r"typedef struct MttsBiasTable \{(.*?)\} MttsBiasTable;", text, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[MTTS_BIAS_RULES_MAX\])?;", tab) == [f[0] for f in capi.MttsBiasTable._fields_]
    assert C.sizeof(capi.MttsBiasTable) == 4 + 8 * bias_spec.RULES_MAX
    for name in ("mtts_set_sampler_bias", "mtts_k_seq_bias", "mtts_k_sample_bias", "mtts_debug_bias_launches"):
        assert name in text and name in capi.exported_symbols()


def test_c_abi_symbols():
    """The built library exports the new entry points."""
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("mtts_set_sampler_bias", "mtts_k_seq_bias", "mtts_k_sample_bias", "mtts_debug_bias_launches"):
        assert hasattr(lib, name), name


# ---- generation_config -----------------------------------------------------------------------------------------------------
def test_config_without_the_four_gives_todays_dicts():
    four = dict(repetition_penalty=1.1, temperature=0.9, top_k=20, top_p=0.8)
    assert ma.GenerationConfig(do_sample=True, **four).channel_settings(8) == ([four] * 8, [True] * 8)
    assert ma.GenerationConfig().channel_settings(8) == ([{}] * 8, [False] * 8)
    assert ma.GenerationConfig(repetition_penalty=1.2).channel_settings(8) == ([dict(repetition_penalty=1.2)] * 8, [False] * 8)
    # HF's conditions: None, m <= 0, m without an eos_token_id
    gc = ma.GenerationConfig(sequence_bias=None, bad_words_ids=None, min_length=0, begin_suppress_tokens=None)
    assert gc.channel_settings(8) == ([{}] * 8, [False] * 8)
    assert ma.GenerationConfig(min_length=40).channel_settings(8) == ([{}] * 8, [False] * 8)
    lay = [dict(temperature=0.7)] * 8
    assert ma.GenerationConfig(do_samples=[True] * 8, layers=lay, bad_words_ids=[[3]]).channel_settings(8) == (lay, [True] * 8)


def test_config_global_branch_and_layers():
    four = dict(sequence_bias={(5,): 0.5, (7, 9): -1.0}, bad_words_ids=[[3, 4]], min_length=40, begin_suppress_tokens=[6])
    layers, ds = ma.GenerationConfig(eos_token_id=7, **four).channel_settings(8)
    assert ds == [False] * 8 and layers == [four] * 8                     # greedy: the processors alone, on all eight channels
    layers, ds = ma.GenerationConfig(do_sample=True, temperature=0.8, eos_token_id=7, **four).channel_settings(8)
    assert ds == [True] * 8 and layers[0]["temperature"] == 0.8 and {k: layers[3][k] for k in four} == four
    arr = sampler_bias(layers, 7)
    assert all(a.n_rules == 3 and a.min_length == 40 and a.n_begin_suppress == 1 for a in arr)
    # the list form of a generation_config.json
    layers, _ = ma.GenerationConfig(sequence_bias=[[[5], 0.5], [[7, 9], -1.0]]).channel_settings(8)
    assert bias_spec.bias_of(layers[0])[0] == [((5,), 0.5), ((7, 9), -1.0)]
    # keyword overrides for one call
    layers, _ = ma.GenerationConfig(eos_token_id=7, **four).channel_settings(8, bad_words_ids=[[1]], min_length=9)
    assert layers[0] == dict(four, bad_words_ids=[[1]], min_length=9)
    # per-channel branch: layers[i] carries them
    lay = [dict(sequence_bias={(5,): 0.5})] + [dict(bad_words_ids=[[3, 4]], min_length=12)] * 7
    layers, ds = ma.GenerationConfig(do_samples=[False] * 8, layers=lay).channel_settings(8)
    assert [a.n_rules for a in sampler_bias(layers)] == [1] * 8 and [a.min_length for a in sampler_bias(layers)] == [0] + [12] * 7


class _Stub(ma.AsteroidTTSInstruct):
    """generate() up to the point where it would touch the device."""

    def __init__(self, gc):
        self.generation_config, self.channels, self.sample_rows, self.sample_seed, self._calls = gc, 8, None, None, 0

    def _get_engine(self, *a, **k):
        raise RuntimeError("device touched")


def test_generate_refuses_before_the_device():
    ids = torch.zeros(1, 12, 8, dtype=torch.long)
    for kw, word in ((dict(sequence_bias={(3,): float("inf")}), "sequence_bias"), (dict(sequence_bias={(-3,): 1.0}), "sequence_bias"),
                     (dict(bad_words_ids=[[3, -2]]), "bad_words_ids"), (dict(min_length=-1), "min_length"),
                     (dict(begin_suppress_tokens=[-1]), "begin_suppress_tokens")):
        with pytest.raises(ValueError, match=r"generate\(\): .*" + word):
            _Stub(ma.GenerationConfig()).generate(ids, max_new_tokens=4, **kw)
    with pytest.raises(ValueError, match="generation_config, channel 2: .*bad_words_ids"):
        lay = [{}] * 2 + [dict(bad_words_ids=[[]])] + [{}] * 5
        _Stub(ma.GenerationConfig(do_samples=[False] * 8, layers=lay)).generate(ids, max_new_tokens=4)
    with pytest.raises(ValueError, match="generation_config, channel 0: .*sequence_bias"):
        _Stub(ma.GenerationConfig(sequence_bias={(4,): float("nan")})).generate(ids, max_new_tokens=4)
    for kw in (dict(sequence_bias={(2,): 1.0}), dict(bad_words_ids=[[1]]), dict(min_length=2), dict(begin_suppress_tokens=[1])):
        with pytest.raises(ValueError, match=r"do_samples set.*layers\[i\]"):
            _Stub(ma.GenerationConfig(do_samples=[True] * 8, layers=[{}] * 8)).generate(ids, max_new_tokens=4, **kw)
    with pytest.raises(RuntimeError, match="device touched"):           # good values reach the engine
        _Stub(ma.GenerationConfig(eos_token_id=7)).generate(ids, max_new_tokens=4, sequence_bias={(3, 4): -0.5}, bad_words_ids=[[0, 1]],
                                                            min_length=3, begin_suppress_tokens=[5])


# ---- host staging and run state under the sanitizers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("c++") is None:
        pytest.skip("c++ is not on the path")
    out = str(tmp_path_factory.mktemp("bias_stage") / "bias_stage_main")
    src = os.path.join(ROOT, "tests", "host", "bias_stage_main.cpp")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return out


@pytest.mark.parametrize("case", ["rules", "bias", "plan", "bufs"])
def test_host_staging_and_run_state(program, case):
    """rules: stage_bias_rules keeps the rules inside the vocabulary, single-token ones first; bias: PendingRun::set_bias
    validates with the channel named, copies the lists and is a one-shot; plan: bias_on / bias_terms are part of the plan's
    equality; bufs: the new StepBufs members take part in the bytewise comparison."""
    r = subprocess.run([program, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1:] == ["ok " + case] and not r.stderr, r.stdout + r.stderr
