"""The plan tells the truth: what mtts_debug_step_plan says a decode step launches (csrc/stepplan.h: describe) against the
launch counters of exactly one such step issued on the stream (MTTS_GRAPHS=0, so every launch counts), on the tiny
synthetic config and on the two-layer bench-width one, under each switch that changes the choice.  And the plan is the
key of a captured step: a read policy that flips in the middle of a run changes the plan, and the step is captured again
without anybody dropping the old graphs.  -m gpu."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402

SWITCHES = ("MTTS_W_SEAL", "MTTS_ATTN_ROW", "MTTS_FOLD_NORM", "MTTS_GEMM_DEPTH", "MTTS_KV_PACK", "MTTS_KV_PACK_MIN", "MTTS_SMALL_ROWS",
            "MTTS_FUSE_QKV_MAX", "MTTS_W_SEAL_HEAD")


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


def _counters():
    lib = capi.lib()
    return dict(depth=int(lib.mtts_debug_gemm_depth_launches()), wseal=int(lib.mtts_debug_wseal_launches()),
                row=int(lib.mtts_debug_attn_row_launches()), fold=int(lib.mtts_debug_fold_norm_launches()))


def _implied(lines, L):
    """Launches of one step by the plan's text: a layer line stands for that launch in each of the L layers, a head line for
    one; "depth", "gateup48" and every sealed GEMM are depth-specialised launches, the fold pair is two launches."""
    n = dict(depth=0, wseal=0, row=0, fold=0)
    for line in lines:
        name, _, text = line.partition(": ")
        words = text.split()
        m = re.fullmatch(r"attn\[(\d+)\.\.(\d+)\]", name)
        if m:
            n["row"] += (int(m.group(2)) - int(m.group(1)) + 1) * (words[0] == "row")
        elif name == "o_proj+gate_up":
            assert words == ["fold"]
            n["fold"] += 2 * L
        elif name in ("qkv", "o_proj", "gate_up", "down", "head0", "heads1_7"):
            times = 1 if name.startswith("head") else L
            n["depth"] += times * bool({"depth", "gateup48", "sealed"} & set(words))
            n["wseal"] += times * ("sealed" in words)
        else:
            assert name in ("pass", "sample"), line
    return n


def _prompts(cfg, B, T, seed):
    rng = np.random.default_rng(seed)
    ids = np.full((B, T, 8), 1024, dtype=np.int64)
    ids[:, :, 0] = rng.integers(0, cfg["vocab_size"] - 10, (B, T))
    return ids, np.ones((B, T), dtype=np.int64)


CONFIGS = {
    # (config, rows, prompt slots): 32 rows x 17 KV pages reach the sealed KV reads' minimum, 32 rows x 8 kv heads fill the device
    "tiny": (lambda: synth.tiny(), 8, 150),
    "bench_width": (lambda: dict(synth.assumed_1p7b(), num_hidden_layers=2), 32, 1047),
}
CASES = {
    "default": ({}, None),
    "w_seal_off": ({"MTTS_W_SEAL": "0"}, None),
    "attn_row_off": ({"MTTS_ATTN_ROW": "0"}, None),
    "fold_norm": ({"MTTS_FOLD_NORM": "1"}, None),
    "gemm_depth_off": ({"MTTS_GEMM_DEPTH": "0"}, None),
    "one_row": ({}, 1),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("which", sorted(CONFIGS))
def test_one_step_launches_what_its_plan_says(monkeypatch, which, case):
    from mtts.engine import Engine
    make, B, T = CONFIGS[which]
    env, rows = CASES[case]
    B = rows or B
    cfg = make()
    L = cfg["num_hidden_layers"]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MTTS_GRAPHS", "0")
    eng = Engine(cfg, max_batch=B, max_seq_len=T + 64)
    for name, t in _rand_weights(cfg, 5):
        eng.bind(name, t)
    ids, mask = _prompts(cfg, B, T, 11)
    eng.begin(ids, mask, T + 16, do_samples=[False] * 8)
    pages = (T - 7 + 1 + 63) // 64                       # the step appends token T - 7 + 1 of every row
    lines = eng.step_plan(pages)
    c0 = _counters()
    eng.step(1)
    steps, _ = eng.sync_state()
    c1 = _counters()
    eng.close()
    assert steps == 1
    got = {k: c1[k] - c0[k] for k in c0}
    print(which, case, lines, got)
    assert lines[0] == "pass: %s B=%d R=32 heads=1 layers=%d" % ("small" if B == 1 else "rows", B, L)
    assert got == _implied(lines, L), lines
    # the switches reach the plan (what each path computes is pinned bitwise by the suites of those paths)
    text = "\n".join(lines)
    if case in ("w_seal_off", "gemm_depth_off", "one_row"):
        assert got["wseal"] == 0 and not re.search(r"^(gate_up|down|head0|heads1_7): .*sealed", text, re.M)
    if case in ("attn_row_off", "one_row"):
        assert got["row"] == 0
    if case in ("gemm_depth_off", "one_row"):
        assert got["depth"] == 0 and got["fold"] == 0
    if which == "bench_width" and case == "default":
        assert lines[2:] == ["qkv: skinny", "attn[0..1]: row sealed", "o_proj: depth", "gate_up: gateup48", "down: depth sealed",
                             "head0: sealed persistent", "heads1_7: sealed persistent"]
    if which == "bench_width" and case == "fold_norm":
        assert got["fold"] == 2 * L and "o_proj+gate_up: fold" in lines
    if which == "bench_width" and case == "attn_row_off":
        assert "attn[0..1]: two_pass fused sealed" in lines


def test_a_changed_plan_is_captured_again(monkeypatch):
    """test_kvpack_gpu's V-policy run (v_proj rows that do not seal: after the first host sync the layers' V reads go back to
    bf16 pages) with the sealed reads on from the first page: the steps before the sync are captured with sealed V reads,
    the steps after it have another plan and are captured again; tokens equal the run that launches every step on the
    stream."""
    from mtts.engine import Engine
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 78, emb_row_sigma=0.6, speech_boost=5.0)
    for k in [k for k in w if k.endswith("v_proj.weight")]:
        w[k] = (w[k] * (2.0 ** (-8.0 * (np.arange(w[k].shape[0]) % 4)))[:, None].astype(np.float32)).astype(np.float32)
    B, T = 2, 700
    ids, mask = _prompts(cfg, B, T, 4)
    pages = (T - 7 + 12 + 63) // 64
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MTTS_KV_PACK_MIN", "1")
    res = {}
    for graphs in ("1", "0"):
        monkeypatch.setenv("MTTS_GRAPHS", graphs)
        eng = Engine(cfg, max_batch=B, max_seq_len=1024)
        eng.bind_state_dict(w)
        eng.begin(ids, mask, T + 40, do_samples=[False] * 8)
        before = eng.step_plan(pages)
        eng.step(4)
        eng.sync_state()
        after = eng.step_plan(pages)
        eng.step(8)
        steps, _ = eng.sync_state()
        res[graphs] = (before, after, steps, eng.read_generated(20), eng.kv_pack_stats())
        eng.close()
    before, after, steps, gen, st = res["1"]
    L = cfg["num_hidden_layers"]
    assert steps == 12 and gen.shape[0] == 12
    assert "attn[0..%d]: two_pass fused sealed" % (L - 1) in before
    assert "attn[0..%d]: two_pass fused k_sealed" % (L - 1) in after
    assert st["k_layers_on"] == L and st["v_layers_on"] == 0
    assert res["0"][:3] == (before, after, steps)
    assert np.array_equal(gen, res["0"][3])
