"""The launching-thread pool of a multi-device handle (hippopt_amd/csrc/multi_pool.h: one worker per shard, hipnlp_multi_set_threads)
on the CPU.  The library runs the pool with hipSetDevice and kernel launches; tests/multi_pool_check/multi_pool_check.cpp runs the SAME
text with a recorder in their place — one call per shard and run, on the bound thread; no job held or called after run() returned;
nothing of an earlier job after stop() and start(); wake-ups across the boundary between polling and sleeping; return codes; the
lifecycle's edges — for 1, 2, 4 and 8 shards and spin_us of 0, 50 and 1e6.  Built twice, plain and with ThreadSanitizer, and run as a
child process: no sanitized code is loaded into this interpreter.  A scenario that does not finish is ended by the program's own
watchdog (exit status 3, the scenario named)."""
import os
import subprocess

import pytest

from emu_build import ROOT

SRC = os.path.join(ROOT, "tests", "multi_pool_check", "multi_pool_check.cpp")
DEPS = [SRC, os.path.join(ROOT, "hippopt_amd", "csrc", "multi_pool.h")]
FLAGS = ["-std=c++17", "-O1", "-g", "-pthread"]
N_LINES = 6 * 12 + 4 * 2 + 4   # six scenarios x 4 shard counts x 3 spin_us, the wake-ups at two spin_us, the lifecycle edges once per shard count


def program(name, extra):
    """tests/_build/<name>, compiled when it is older than the program's text or the pool's (emu_build.build's check, for an executable)"""
    exe = os.path.join(ROOT, "tests", "_build", name)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe + ".tmp", SRC])
        os.replace(exe + ".tmp", exe)
    return exe


@pytest.mark.parametrize("name,extra", [("multi_pool_check", []), ("multi_pool_check_tsan", ["-fsanitize=thread"])])
def test_pool_lifecycle_on_the_cpu(name, extra):
    exe = program(name, extra)
    env = dict(os.environ, TSAN_OPTIONS="exitcode=66 halt_on_error=0")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    print(run.stdout)
    print(run.stderr)
    assert "ThreadSanitizer" not in run.stderr and "ThreadSanitizer" not in run.stdout, run.stderr[:4000]
    assert run.returncode == 0, (run.returncode, [l for l in run.stdout.splitlines() if not l.startswith("ok ")], run.stderr[:2000])
    lines = run.stdout.splitlines()
    assert lines[-1].startswith("passed: 0 failing")
    assert sum(l.startswith("ok ") for l in lines) == N_LINES == len(lines) - 1
