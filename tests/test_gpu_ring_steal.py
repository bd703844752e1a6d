"""The ring fold's round scheduler (csrc/cc_kernels.hpp RingSteal: a static part, a stealable tail
handed out by per-workgroup counters, two counter sets alternating between launches), one
subprocess per environment: the library reads its debug variables once per process.

tests/ring_steal_check.py folds two streams window by window — launches of alternating sizes
(4 edges to 2^23: one workgroup and a partial wave, a last workgroup that owns one group, a ragged
last row, launches that are all tickets, launches with static rows before the tickets) and a stream
in which 8 workgroups own all the unions, so their tails are expected to be stolen — on a plain
and a track_marks handle with int32 and int64 ids, every window's checksum and the final dense
labels against the C oracle. The streams and the oracle's results are
made once (the `reference` fixture) and shared by all environments.

* test_ring_steal_parity: the ring fold forced (GSGPU_FOLD_MODE=ring), the ring fold with its warm
  set from 2^20 ids (GSGPU_RING_MIN_BITS=20), the same with the static loop (GSGPU_RING_STEAL=0), and
  the same with a stealable tail of 2 rows (GSGPU_RING_STEAL=2: the 2^22-edge launches then run 2
  static rows and 2 rows of tickets, the 2^23-edge launch 6 and 2).
* test_ring_steal_every_edge_once: with GSGPU_FOLD_STATS the fold statistics report `valid` equal
  to the window's edges for every window (one ring launch each past the young forest): no round is
  skipped or handed out twice.
"""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "ring_steal_check.py")

ENVS = {
    "ring_forced": {"GSGPU_FOLD_MODE": "ring"},
    "ring_warm_from_2^20": {"GSGPU_RING_MIN_BITS": "20"},
    "ring_warm_from_2^20_static": {"GSGPU_RING_MIN_BITS": "20", "GSGPU_RING_STEAL": "0"},
    "ring_warm_from_2^20_tail_2": {"GSGPU_RING_MIN_BITS": "20", "GSGPU_RING_STEAL": "2"},
}


def _env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSGPU_")}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ring_steal") / "ref.npz")
    subprocess.check_call([sys.executable, CHECK, "--make-ref", path], env=_env({}), timeout=300)
    return path


def _check(reference, extra):
    p = subprocess.run([sys.executable, CHECK, "--ref", reference], env=_env(extra), timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    r = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1])
    bad = [c for c in r["cases"] if not c["ok"]]
    assert r["ok"] and not bad and len(r["cases"]) == 8, bad
    return r, p.stderr.decode()


@pytest.mark.parametrize("name", list(ENVS))
def test_ring_steal_parity(reference, name):
    _check(reference, ENVS[name])


def test_ring_steal_every_edge_once(reference):
    r, err = _check(reference, {"GSGPU_RING_MIN_BITS": "20", "GSGPU_FOLD_STATS": "1"})
    valid = [int(v) for v in re.findall(r"\[gsgpu fold-stats\] valid=(\d+)", err)]
    valid = [v for v in valid if v]                      # (reports with no fold since the last one)
    print(valid)
    assert valid == r["stats_valid"]
