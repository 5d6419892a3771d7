"""The engine's HIP-free host code -- the KV page pool (csrc/kvpool.h) and the prompt stager (csrc/staging.h) -- run on
the CPU under AddressSanitizer and UBSan.  tests/host/pool_stage_main.cpp is a stand-alone program that includes the two
headers and nothing of HIP; it is built here with the host compiler into a temporary directory and run as a child
process, once per case.  The cases restate on the host what the GPU suite pins through the engine (test_robustness_gpu,
test_takes_gpu, test_longctx_gpu, the *_leaves_the_engine_untouched tests): hand-out order, batches of at most 31 edits
without a repeated index, a grow that runs dry, shared pages, and the borrow of mtts_score."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "pool_stage_main.cpp")

pytestmark = pytest.mark.skipif(shutil.which("c++") is None, reason="c++ is not on the path")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_pool") / "pool_stage_main")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return out


def _run(program, case):
    """The case's output lines without the closing "ok <case>"; exit status 0 and that line are asserted."""
    r = subprocess.run([program, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines and lines[-1] == "ok " + case, r.stdout
    return lines[:-1]


def _shuffled_order(total, seed):
    """The order a pool shuffled with `seed` hands its pages out in, restated from the definition: free[i] = total-1-i,
    a Fisher-Yates pass from the back driven by a 64-bit LCG, pages taken from the back."""
    mask = (1 << 64) - 1
    free = [total - 1 - i for i in range(total)]
    x = 0x9E3779B97F4A7C15 ^ seed
    for i in range(total - 1, 0, -1):
        x = (x * 6364136223846793005 + 1442695040888963407) & mask
        j = (x >> 33) % (i + 1)
        free[i], free[j] = free[j], free[i]
    return free[::-1]


def test_hand_out_order(program):
    (line,) = _run(program, "pool_order")                 # the fresh 9-page pool's 0..8 is asserted by the program
    order = [int(v) for v in line.split()[1:]]
    assert sorted(order) == list(range(40))
    assert order == _shuffled_order(40, 17)
    assert order != list(range(40))


def test_batches_of_a_long_grow(program):
    assert _run(program, "pool_batches") == ["batches 3"]          # 70 pages: 31 + 31 + 8


def test_dry_mid_grow_then_recovery(program):
    assert _run(program, "pool_dry") == ["free 3"]


def test_need_above_the_row_width(program):
    assert _run(program, "pool_wide") == ["error slot 1 needs 7 KV pages, a sequence holds at most 6 (max_seq_len 320)"]


def test_shared_pages(program):
    assert _run(program, "pool_shares") == ["free 5"]


def test_borrow_leaves_the_pool_as_it_was(program):
    assert _run(program, "pool_borrow") == ["free 18"]


def test_stager_lengths_around_the_tile(program):
    assert _run(program, "stage_lengths") == ["mpad 256"]


def test_stager_single_row(program):
    assert _run(program, "stage_one") == ["mpad 128"]


def test_stager_shifted_labels(program):
    assert _run(program, "stage_labels") == ["labels ok"]


def test_stager_refusals_keep_their_texts(program):
    assert _run(program, "stage_refusals") == [
        "negative: -1: token -1 out of range on channel 3",
        "speech: -1: token 100 out of range on channel 5",
        "text: -1: token 300 out of range on channel 0",
        "left hole: -1: attention_mask of row 2 is not left-padded",
        "left empty: -1: row 1 has no real token in the first T-7 slots",
        "right left-padded: -1: attention_mask of row 3 is left-padded: mtts_score takes right-padded or unpadded rows (ones, then zeros)",
        "right hole: -1: attention_mask of row 4 is not ones followed by zeros (right-padded or unpadded rows only)",
        "tail: -1: token 100 out of range on channel 6 (delayed tail)",
    ]


def test_bitmap_and_tail(program):
    (line,) = _run(program, "stage_bitmap_tail")
    assert line.startswith("bits ")
