"""The rendezvous behind the per-party entry points (csrc/party_rdv.hpp: k local callers of a round become one rank call)
as a stand-alone host program, tests/native/party_rdv_test.cpp, built three ways: plain, with ThreadSanitizer, and with
AddressSanitizer + UndefinedBehaviorSanitizer.  The header has no HIP in it, so nothing but the host compiler is needed and
nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "party_rdv_test.cpp")
HDR = os.path.join(ROOT, "zk-saas_amd", "csrc", "party_rdv.hpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
FLAGS = {"plain": ["-O2"],
         "tsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=thread"],
         "asan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def _cxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    pytest.skip("no host C++ compiler")


def _build(kind):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "party_rdv_test_" + kind)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        cmd = [_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[kind] + [
            "-I" + os.path.join(ROOT, "zk-saas_amd", "csrc"), SRC, "-o", exe, "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(kind, args):
    env = dict(os.environ)
    env["TSAN_OPTIONS"] = "halt_on_error=1 exitcode=66 second_deadlock_stack=1"
    env["ASAN_OPTIONS"] = "exitcode=67"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1 halt_on_error=1"
    r = subprocess.run([_build(kind)] + args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "%s %s: exit %d\n%s" % (kind, args, r.returncode, (r.stderr or r.stdout)[-4000:])


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", ["plain", "tsan", "asan"])
def test_rounds_one_issue_per_round_in_party_order(kind, k):
    """k parties x three slots, one thread each, 200 rounds per slot with randomised arrival order: the callback runs exactly
    once per round with the k records of that round in party order, every caller gets its code, sequence numbers hold."""
    _run(kind, ["rounds", str(k)])


@pytest.mark.parametrize("kind", ["plain", "tsan", "asan"])
def test_a_differing_record_is_bad_input_for_everyone(kind):
    _run(kind, ["mismatch"])


@pytest.mark.parametrize("kind", ["plain", "tsan", "asan"])
def test_a_party_that_stays_away_fails_the_slot_within_the_deadline(kind):
    _run(kind, ["timeout"])


@pytest.mark.parametrize("kind", ["plain", "tsan", "asan"])
def test_a_second_thread_in_the_same_party_and_slot_is_refused(kind):
    _run(kind, ["twice"])
