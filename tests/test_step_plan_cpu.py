"""How a pass chooses its kernels -- plan_step of csrc/stepplan.h -- run on the CPU under AddressSanitizer and UBSan.
tests/host/step_plan_main.cpp is a stand-alone program that includes that header and nothing of HIP; it is built here with
the host compiler into a temporary directory and run as a child process, once per case.  `plan key=value ...` prints
describe() of the plan for the bench width (32 dialogues, 8 kv heads, 256 compute units, 64 KV pages, default switches,
down_proj and the heads reading their sealed twins) with the given values changed.  The cases restate on the host what
the GPU suite pins through the engine bitwise and by launch counters (test_gemm_depth_gpu, test_wseal_gpu,
test_fold_norm_gpu, test_attn_row_gpu, test_kvpack_gpu, the small-batch and fused-epilogue tests of test_engine_gpu)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "step_plan_main.cpp")

pytestmark = pytest.mark.skipif(shutil.which("c++") is None, reason="c++ is not on the path")

L = 28
LDS = 160 * 1024          # the program's row_lds_limit


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("step_plan") / "step_plan_main")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return out


def _run(program, *args):
    """The case's output lines without the closing "ok <case>"; exit status 0 and that line are asserted."""
    r = subprocess.run([program] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines and lines[-1] == "ok " + args[0], r.stdout
    return lines[:-1]


def _plan(program, **kw):
    """describe() as {group: text} plus the attention lines in order as a list under "attn"."""
    out, attn = {}, []
    for line in _run(program, "plan", *["%s=%s" % kv for kv in kw.items()]):
        name, _, text = line.partition(": ")
        if name.startswith("attn["):
            attn.append((name, text))
        else:
            assert name not in out, line
            out[name] = text
    out["attn"] = attn
    return out


def _lds_bytes(G, pk, pages):
    """attn_row_lds_bytes restated: q, the new K / V rows, per wave (12) the rescaled q (sealed pages only) and the
    probability pairs, per page 8 B of pairs + 128 B of scores, per chunk of 8 pages 4 item vectors of 512 B, all x G."""
    return G * 256 + 512 + (12 * G * 256 if pk else 0) + 12 * G * 128 + G * pages * (8 + 128) + 4 * ((pages + 7) // 8) * G * 512


ALL = "attn[0..%d]" % (L - 1)


def test_bench_width(program):
    p = _plan(program)
    assert p == {"pass": "rows B=32 R=32 heads=1 layers=28", "sample": "ch0_greedy topk=0", "qkv": "skinny",
                 "attn": [(ALL, "row sealed")], "o_proj": "depth", "gate_up": "gateup48", "down": "depth sealed",
                 "head0": "sealed persistent", "heads1_7": "sealed persistent"}
    assert _plan(program, w_seal_head=0)["head0"] == "sealed"


def test_small_path_and_its_bounds(program):
    for B in (1, 4):
        p = _plan(program, B=B)
        assert p["pass"] == "small B=%d R=32 heads=1 layers=28" % B
        assert {p[g] for g in ("qkv", "o_proj", "gate_up", "down", "head0", "heads1_7")} == {"small"}
        assert p["attn"] == [(ALL, "two_pass fused")]               # 4 x 64 pages: below the sealed reads' minimum
    for kw in ({"B": 5}, {"B": 1, "lora": 1}, {"B": 1, "small_fits": 0}, {"B": 1, "small_rows": 0}):
        assert _plan(program, **kw)["pass"].startswith("rows B=%d R=32" % kw["B"]), kw
    assert _plan(program, B=3, small_rows=2)["pass"].startswith("rows")
    assert _plan(program, B=2, small_rows=2)["pass"].startswith("small")
    # the small path's attention follows the same thresholds (it never takes the row kernel)
    assert _plan(program, B=4, pages=128, attn_row=2)["attn"] == [(ALL, "two_pass fused sealed")]
    assert _plan(program, B=4, pages=641)["attn"] == [(ALL, "two_pass epilogue sealed")]


def test_lora(program):
    base, p = _plan(program), _plan(program, lora=1)
    assert p["pass"] == base["pass"] and p["attn"] == base["attn"]
    assert (p["qkv"], p["o_proj"], p["gate_up"], p["down"]) == ("skinny +lora", "depth +lora", "skinny slab +lora", "depth +lora")
    assert p["head0"] == p["heads1_7"] == "skinny"
    assert "o_proj+gate_up" not in _plan(program, lora=1, fold_norm=1, wseal_on=0)
    assert "sealed" not in p["gate_up"] and "sealed" not in _plan(program, lora=1, wseal_kind=15, wseal_on=15)["gate_up"]


def test_thresholds_on_both_sides(program):
    # q/k/v epilogue inside the attention kernels while rows x pages <= 2560 (the two-pass form: MTTS_ATTN_ROW=0)
    assert _plan(program, attn_row=0, pages=80)["attn"] == [(ALL, "two_pass fused sealed")]
    assert _plan(program, attn_row=0, pages=81)["attn"] == [(ALL, "two_pass epilogue sealed")]
    assert _plan(program, attn_row=0, B=31, pages=82, fuse_qkv_max=31 * 82)["attn"] == [(ALL, "two_pass fused sealed")]
    # sealed KV reads from 512 rows x pages up
    assert _plan(program, pages=16)["attn"] == [(ALL, "row sealed")]
    assert _plan(program, pages=15)["attn"] == [(ALL, "row")]
    assert _plan(program, B=31, pages=16)["attn"] == [(ALL, "two_pass fused")]
    assert _plan(program, kv_pack=0)["attn"] == [(ALL, "row")]
    # the row kernel by the shape: its blocks fill the machine
    assert _plan(program, B=32, n_cus=256)["attn"] == [(ALL, "row sealed")]
    assert _plan(program, B=31, n_cus=256)["attn"] == [(ALL, "two_pass fused sealed")]
    assert _plan(program, B=32, n_cus=257)["attn"] == [(ALL, "two_pass fused sealed")]
    assert _plan(program, B=31, attn_row=2)["attn"] == [(ALL, "row sealed")]
    assert _plan(program, B=32, attn_row=0)["attn"] == [(ALL, "two_pass fused sealed")]
    assert _plan(program, B=128, nkv=2, attn_row=1)["attn"] == [(ALL, "row sealed")]
    # nothing fits an engine whose device refused the LDS
    assert _plan(program, attn_row=2, row_lds_limit=0)["attn"] == [(ALL, "two_pass fused sealed")]


def test_prefill_passes(program):
    for heads in (0, 2):
        p = _plan(program, heads=heads, R=2048, B=4, pages=8)
        assert p["pass"] == "rows B=4 R=2048 heads=%d layers=28" % heads and "sample" not in p
        assert (p["qkv"], p["o_proj"], p["gate_up"], p["down"]) == ("tile",) * 4
        assert p["attn"] == [(ALL, "prefill mfma")]
        assert ("head0" in p) == (heads == 2)
    assert _plan(program, heads=2, R=128, B=4, pages=8, pf_mfma_pages=8)["attn"] == [(ALL, "prefill mfma")]
    assert _plan(program, heads=2, R=128, B=4, pages=7, pf_mfma_pages=8)["attn"] == [(ALL, "two_pass epilogue")]
    # the end of a prefill packs the dialogues' last rows into tiles of their own: one tile reads the heads sealed
    assert _plan(program, heads=2, R=2048, B=32)["head0"] == "sealed persistent"
    assert _plan(program, heads=2, R=2048, B=33)["head0"] == "skinny x2"
    # a prefill never takes the small path, a sealed layer GEMM, the fold pair or sealed pages
    p = _plan(program, heads=2, R=32, B=1, pages=600, fold_norm=1, wseal_kind=15, wseal_on=14)
    assert p["pass"].startswith("rows") and p["down"] == "tile" and "o_proj+gate_up" not in p and p["attn"] == [(ALL, "prefill mfma")]


def test_mixed_layer_policy_and_the_lds_bound(program):
    p = _plan(program, k_off=3)                       # layer 3: K back to bf16 reads, V sealed
    assert p["attn"] == [("attn[0..2]", "row sealed"), ("attn[3..3]", "two_pass fused v_sealed"), ("attn[4..27]", "row sealed")]
    p = _plan(program, v_off="0,27")
    assert p["attn"] == [("attn[0..0]", "two_pass fused k_sealed"), ("attn[1..26]", "row sealed"), ("attn[27..27]", "two_pass fused k_sealed")]
    assert _plan(program, k_off=5, v_off=5)["attn"] == [("attn[0..4]", "row sealed"), ("attn[5..5]", "row"), ("attn[6..27]", "row sealed")]
    # the row kernel ends where its LDS exceeds what a block may take: the bound from the formula, sealed and bf16 pages
    for pk, kw in ((True, {}), (False, {"kv_pack": 0})):
        last = max(pg for pg in range(1, 2000) if _lds_bytes(4, pk, pg) <= LDS)
        assert _lds_bytes(4, pk, last) <= LDS < _lds_bytes(4, pk, last + 1)
        assert int(_run(program, "lds", 4, int(pk), last)[0]) == _lds_bytes(4, pk, last)
        assert _plan(program, pages=last, **kw)["attn"][0][1].startswith("row")
        assert _plan(program, pages=last + 1, **kw)["attn"][0][1].startswith("two_pass epilogue")
    # a layer on bf16 pages needs less LDS than its sealed neighbours: it keeps the row kernel one step longer
    last = max(pg for pg in range(1, 2000) if _lds_bytes(4, True, pg) <= LDS)
    assert _lds_bytes(4, False, last + 1) <= LDS
    assert _plan(program, pages=last + 1, k_off=1, v_off=1)["attn"] == [
        ("attn[0..0]", "two_pass epilogue sealed"), ("attn[1..1]", "row"), ("attn[2..27]", "two_pass epilogue sealed")]


def test_depth_fold_and_row_tiles(program):
    p = _plan(program, gemm_depth=0, fold_norm=1, wseal_kind=15, wseal_on=15)
    assert {p[g] for g in ("qkv", "o_proj", "gate_up", "down", "head0", "heads1_7")} == {"skinny"}
    # the pair only at one row tile, without adapters, gate/up not sealed, and the shape it is built for
    assert _plan(program, fold_norm=1)["o_proj+gate_up"] == "fold"
    assert "o_proj" not in _plan(program, fold_norm=1) and "gate_up" not in _plan(program, fold_norm=1)
    for kw in ({"B": 33}, {"lora": 1}, {"wseal_kind": 15, "wseal_on": 15}, {"wseal_on": 15}, {"fold_shape": 0}, {"fold_norm": 0},
               {"heads": 2, "R": 32}):
        kw = dict({"fold_norm": 1}, **kw)
        assert "o_proj+gate_up" not in _plan(program, **kw), kw
    assert _plan(program, wseal_kind=15, wseal_on=15)["gate_up"] == "gateup48 sealed"
    assert _plan(program, wseal_kind=14, wseal_on=15)["gate_up"] == "gateup48"        # no twin: nothing to read
    assert _plan(program, wseal_on=0)["down"] == "depth"
    # two row tiles read nothing sealed and take no depth-specialised kernel
    p = _plan(program, B=33, wseal_kind=15, wseal_on=15)
    assert p["pass"] == "rows B=33 R=64 heads=1 layers=28"
    assert {p[g] for g in ("qkv", "o_proj", "gate_up", "down", "head0", "heads1_7")} == {"skinny x2"}
    assert _plan(program, B=128, wseal_kind=15, wseal_on=15)["down"] == "skinny x4"


def test_f32_engine_and_sampler_variants(program):
    p = _plan(program, f32=1, forced=1, ch0_sampled=1, scores=1, topk=5)
    assert p == {"pass": "f32 B=32 R=32 heads=1 layers=0", "sample": "ch0_sampled scores forced topk=5", "attn": []}
    assert _plan(program, topk=2)["sample"] == "ch0_greedy topk=2"


def test_plans_compare_equal_exactly_when_they_describe_alike(program):
    """The plan is the key of a captured step: over every combination of the values above (rows 1 / 4 / 5 / 31 / 32 / 33,
    pages 15 / 16 / 80 / 81, adapters, MTTS_ATTN_ROW 0 / 1 / 2, MTTS_GEMM_DEPTH, MTTS_FOLD_NORM, three weight policies, a
    layer with K off, two sampler variants) two states' plans are == exactly when describe() and the sampler variants
    agree -- the program fails otherwise -- and the number of distinct plans is what it was when this was written."""
    assert _run(program, "sweep") == ["states 6912", "distinct 328"]
