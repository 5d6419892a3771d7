"""What a run starts with and what a captured step holds on to -- csrc/runstate.h -- run on the CPU under AddressSanitizer,
LeakSanitizer and UBSan.  tests/host/run_state_main.cpp is a stand-alone program that includes that header and nothing of
HIP; it is built here with the host compiler into a temporary directory and run as a child process, once per case.  The
graph handles of its cache cases are heap allocations: a captured step that is never destroyed, or destroyed twice, ends
the child with the sanitizer's report.  tests/test_run_state_gpu.py pins the same rules through the engine."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "run_state_main.cpp")

pytestmark = pytest.mark.skipif(shutil.which("c++") is None, reason="c++ is not on the path")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("run_state") / "run_state_main")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return out


def _run(program, case):
    r = subprocess.run([program, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1:] == ["ok " + case] and not r.stderr, r.stdout + r.stderr


def test_take_consumes_the_one_shots_and_copies_the_sticky_ones(program):
    """After each set_* alone and after all of them: the take carries the setting, the next take the default; output_scores
    and top_logprobs stay through every take; a take whose check fails has consumed the one-shots all the same."""
    _run(program, "options")


def test_every_size_mismatch_gives_its_message(program):
    """Row adapters count the prompts, row ids the rows (prompts x takes), the batch fits max_batch (no product of an
    unchecked B is formed: UBSan), a forced replay has no takes; the texts and their order are the engine's."""
    _run(program, "sizes")


def test_a_slot_adapter_is_consumed_once_and_alone(program):
    _run(program, "slots")


def test_a_hit_needs_plan_pages_and_every_byte_of_the_buffers(program):
    """One differing pointer or int of StepBufs misses: swept over every byte of the struct, which has no padding
    (asserted at compile time), and again member by member."""
    _run(program, "key")


def test_insert_with_new_buffers_destroys_exactly_the_stale_steps(program):
    """... once each and in order, also when only a size beside an unchanged address differs; clear() and the cache's end
    destroy the rest; nothing leaks, nothing is freed twice."""
    _run(program, "stale")


def test_the_257th_insert_empties_the_cache_first(program):
    _run(program, "cap")


def test_an_unknown_case_is_an_error(program):
    assert subprocess.run([program, "nothing"], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 2
