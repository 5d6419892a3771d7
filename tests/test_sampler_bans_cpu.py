"""Hard bans (no_repeat_ngram_size, suppress_tokens, min_new_tokens): the rule, the marshalling and the host staging, on the
CPU.  mtts/ban_spec.py is held against the installed transformers' own processors (tests/bans_ref.py);
tests/host/ban_stage_main.cpp runs csrc/staging.h and csrc/runstate.h under AddressSanitizer and UBSan as a child process.
tests/test_sampler_bans_gpu.py holds the kernels and the engine against the same reference."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

from mtts import ban_spec, capi  # noqa: E402
from mtts.engine import sampler_bans, sampler_floors  # noqa: E402
import modeling_asteroid as ma  # noqa: E402

import bans_ref as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule against HF --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 152697])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 16])
def test_ngram_rule_is_hfs(V, n):
    """Lengths 0, n-1, n, n+1 and 300 over alphabets of 3..12 symbols (matches are many), symbols spread over the whole
    vocabulary; with the shared suppress list on top."""
    rng = np.random.default_rng(100 * n + V % 97)
    hits = 0
    for length in (0, n - 1, n, n + 1, 300):
        for k in (3, 5, 12):
            alphabet = rng.choice(V, k, replace=False)
            h = rng.choice(alphabet, length) if length else np.zeros(0, dtype=np.int64)
            for layer in (dict(no_repeat_ngram_size=n), dict(no_repeat_ngram_size=n, suppress_tokens=br.SUPPRESS)):
                want = br.hf_ban_row(h, V, layer)
                got = ban_spec.banned_mask(h, 0, V, layer)
                assert np.array_equal(got, want), (V, n, length, k, np.flatnonzero(got != want)[:8])
                hits += int(got.sum())
    assert hits > 0


@pytest.mark.parametrize("V", [1025, 152697])
def test_suppress_and_min_new_tokens_are_hfs(V):
    """One list with ids on both sides of 1025: those outside the vocabulary are ignored.  min_new_tokens = m bans eos while
    g < m + 7: checked at g = m + 6 (banned) and g = m + 7 (free), where the vocabulary holds eos."""
    rng = np.random.default_rng(5 + V % 97)
    base, eos = 11, 999 if V == 1025 else 151643
    want_ids = [t for t in br.SUPPRESS if t < V]
    got = ban_spec.banned_mask([], 0, V, dict(suppress_tokens=br.SUPPRESS))
    assert np.array_equal(np.flatnonzero(got), np.array(sorted(want_ids)))
    assert np.array_equal(got, br.hf_ban_row(np.zeros(0, dtype=np.int64), V, dict(suppress_tokens=br.SUPPRESS)))
    for m in (1, 5):
        layer = dict(min_new_tokens=m, suppress_tokens=br.SUPPRESS)
        for g in (0, m + 6, m + 7, m + 20):
            h = rng.integers(0, V, base + g)
            want = br.hf_ban_row(h, V, layer, step=g, eos_token_id=eos, base=base)
            got = ban_spec.banned_mask(h, g, V, layer, eos_token_id=eos)
            assert np.array_equal(got, want), (V, m, g)
            assert bool(got[eos]) == (g < m + 7)
    # an eos outside the vocabulary bans nothing; without an eos the processor is absent
    assert not ban_spec.banned_mask([], 0, 1025, dict(min_new_tokens=3), eos_token_id=151643).any()
    assert not ban_spec.banned_mask([], 0, 1025, dict(min_new_tokens=3)).any()


def test_ban_words_layout():
    m = np.zeros(1025, dtype=bool)
    m[[0, 31, 32, 1024]] = True
    w = ban_spec.ban_words(m)
    assert w.dtype == np.uint32 and w.shape == (33,)
    assert w[0] == (1 | 1 << 31) and w[1] == 1 and w[32] == 1 and w[2:32].sum() == 0


# ---- values and marshalling -----------------------------------------------------------------------------------------------
def test_bad_values_name_the_channel():
    for bad, word in ((dict(no_repeat_ngram_size=17), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
                      (dict(suppress_tokens=[4, -1]), "suppress_tokens"), (dict(min_new_tokens=-3), "min_new_tokens"),
                      (dict(no_repeat_ngram_size=2.0), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=True), "no_repeat_ngram_size"),
                      (dict(suppress_tokens=7), "suppress_tokens"), (dict(suppress_tokens="12"), "suppress_tokens")):
        layers = [{}] * 5 + [bad] + [{}] * 2
        with pytest.raises(ValueError, match=re.escape("layers[5]: ") + ".*" + word):
            sampler_bans(layers)
    assert ban_spec.check_ban("no_repeat_ngram_size", 16) == 16 and ban_spec.check_ban("no_repeat_ngram_size", None) == 0
    assert ban_spec.bans_of(None) == (0, 0, []) and ban_spec.bans_of(dict(suppress_tokens=[])) == (0, 0, [])


def test_marshalling():
    assert sampler_bans(None) is None and sampler_bans([{}] * 8) is None
    assert sampler_bans([dict(no_repeat_ngram_size=0, suppress_tokens=[], min_new_tokens=0, temperature=0.5)] * 8) is None
    layers = [dict(no_repeat_ngram_size=3, suppress_tokens=[5, 2000])] + [dict(min_new_tokens=4)] + [{}] * 5 + [dict(suppress_tokens=(9,))]
    arr = sampler_bans(layers)
    assert [a.no_repeat_ngram_size for a in arr] == [3, 0, 0, 0, 0, 0, 0, 0]
    assert [a.min_new_tokens for a in arr] == [0, 4, 0, 0, 0, 0, 0, 0]
    assert [a.n_suppress for a in arr] == [2, 0, 0, 0, 0, 0, 0, 1]
    assert [arr[0].suppress[i] for i in range(2)] == [5, 2000] and arr[7].suppress[0] == 9
    # greedy channels carry their bans: the marshalling does not look at do_samples
    assert sampler_floors(layers, [False] * 8) is None


def test_struct_layout_matches_the_header():
    text = open(os.path.join(ROOT, "include", "mtts.h")).read()
    body = re.search(r"typedef struct MttsSamplerBans \{(.*?)\} MttsSamplerBans;", text, re.S).group(1)
    fields = re.findall(r"^\s*(const int32_t\*|int32_t)\s+(\w+);", body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in capi.MttsSamplerBans._fields_]
    for (ctype, name), (_, py) in zip(fields, capi.MttsSamplerBans._fields_):
        assert py is (C.POINTER(C.c_int32) if ctype.endswith("*") else C.c_int32), name
    assert C.sizeof(capi.MttsSamplerBans) == 24 and capi.MttsSamplerBans.suppress.offset == 16
    assert re.search(r"#define MTTS_NGRAM_MAX (\d+)", text).group(1) == str(ban_spec.NGRAM_MAX)
    for name in ("mtts_set_sampler_bans", "mtts_k_ngram_ban", "mtts_k_sample_bans", "mtts_debug_ban_launches"):
        assert name in text and name in capi.exported_symbols()


# ---- generation_config -----------------------------------------------------------------------------------------------------
def test_config_without_bans_gives_todays_dicts():
    four = dict(repetition_penalty=1.1, temperature=0.9, top_k=20, top_p=0.8)
    assert ma.GenerationConfig(do_sample=True, **four).channel_settings(8) == ([four] * 8, [True] * 8)
    assert ma.GenerationConfig().channel_settings(8) == ([{}] * 8, [False] * 8)
    assert ma.GenerationConfig(repetition_penalty=1.2).channel_settings(8) == ([dict(repetition_penalty=1.2)] * 8, [False] * 8)
    # HF's conditions: n <= 0, m <= 0, m without an eos_token_id, no list
    gc = ma.GenerationConfig(no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None)
    assert gc.channel_settings(8) == ([{}] * 8, [False] * 8)
    assert ma.GenerationConfig(min_new_tokens=4).channel_settings(8) == ([{}] * 8, [False] * 8)
    lay = [dict(temperature=0.7)] * 8
    assert ma.GenerationConfig(do_samples=[True] * 8, layers=lay, no_repeat_ngram_size=3).channel_settings(8) == (lay, [True] * 8)


def test_config_global_branch_greedy_and_sampled():
    bans = dict(no_repeat_ngram_size=3, suppress_tokens=[5, 2000], min_new_tokens=4)
    layers, ds = ma.GenerationConfig(eos_token_id=7, **bans).channel_settings(8)
    assert ds == [False] * 8 and layers == [bans] * 8                     # greedy: the bans alone
    layers, ds = ma.GenerationConfig(eos_token_id=7, repetition_penalty=1.3, **bans).channel_settings(8)
    assert layers == [dict(repetition_penalty=1.3, **bans)] * 8
    layers, ds = ma.GenerationConfig(do_sample=True, temperature=0.8, eos_token_id=7, **bans).channel_settings(8)
    assert ds == [True] * 8 and layers[0]["temperature"] == 0.8 and {k: layers[3][k] for k in bans} == bans
    arr = sampler_bans(layers)
    assert all(a.no_repeat_ngram_size == 3 and a.min_new_tokens == 4 and a.n_suppress == 2 for a in arr)
    # keyword overrides for one call
    layers, _ = ma.GenerationConfig(eos_token_id=7, **bans).channel_settings(8, no_repeat_ngram_size=2, suppress_tokens=[1])
    assert layers[0] == dict(no_repeat_ngram_size=2, suppress_tokens=[1], min_new_tokens=4)
    # per-channel branch: layers[i] carries them
    lay = [dict(no_repeat_ngram_size=3)] + [dict(no_repeat_ngram_size=2, suppress_tokens=[1024])] * 7
    layers, ds = ma.GenerationConfig(do_samples=[False] * 8, layers=lay).channel_settings(8)
    assert [a.no_repeat_ngram_size for a in sampler_bans(layers)] == [3] + [2] * 7


class _Stub(ma.AsteroidTTSInstruct):
    """generate() up to the point where it would touch the device."""

    def __init__(self, gc):
        self.generation_config, self.channels, self.sample_rows, self.sample_seed, self._calls = gc, 8, None, None, 0

    def _get_engine(self, *a, **k):
        raise RuntimeError("device touched")


def test_generate_refuses_before_the_device():
    ids = torch.zeros(1, 12, 8, dtype=torch.long)
    for kw, word in ((dict(no_repeat_ngram_size=17), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
                     (dict(suppress_tokens=[3, -2]), "suppress_tokens"), (dict(min_new_tokens=-1), "min_new_tokens")):
        with pytest.raises(ValueError, match=r"generate\(\): .*" + word):
            _Stub(ma.GenerationConfig()).generate(ids, max_new_tokens=4, **kw)
    with pytest.raises(ValueError, match="generation_config, channel 2: .*no_repeat_ngram_size"):
        lay = [{}] * 2 + [dict(no_repeat_ngram_size=17)] + [{}] * 5
        _Stub(ma.GenerationConfig(do_samples=[False] * 8, layers=lay)).generate(ids, max_new_tokens=4)
    with pytest.raises(ValueError, match="generation_config, channel 0: .*suppress_tokens"):
        _Stub(ma.GenerationConfig(suppress_tokens=[-4])).generate(ids, max_new_tokens=4)
    for kw in (dict(no_repeat_ngram_size=2), dict(suppress_tokens=[1]), dict(min_new_tokens=2)):
        with pytest.raises(ValueError, match="do_samples set.*put the floors there"):
            _Stub(ma.GenerationConfig(do_samples=[True] * 8, layers=[{}] * 8)).generate(ids, max_new_tokens=4, **kw)
    with pytest.raises(RuntimeError, match="device touched"):           # good values reach the engine
        _Stub(ma.GenerationConfig(eos_token_id=7)).generate(ids, max_new_tokens=4, no_repeat_ngram_size=16, suppress_tokens=[0], min_new_tokens=3)


# ---- host staging and run state under the sanitizers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("c++") is None:
        pytest.skip("c++ is not on the path")
    out = str(tmp_path_factory.mktemp("ban_stage") / "ban_stage_main")
    src = os.path.join(ROOT, "tests", "host", "ban_stage_main.cpp")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return out


@pytest.mark.parametrize("case", ["history", "static", "bans", "bufs"])
def test_host_staging_and_run_state(program, case):
    """history: stage_history is the bitmap's token stream, a left-padded row included; static: ids inside the vocabulary
    only; bans: PendingRun::set_bans validates with the channel named and is a one-shot; bufs: the new StepBufs members take
    part in the bytewise comparison."""
    r = subprocess.run([program, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1:] == ["ok " + case] and not r.stderr, r.stdout + r.stderr
