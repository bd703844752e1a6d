"""Structured streams through the ring fold and its warm set, one subprocess per environment (the
library reads its debug variables once per process).

tests/structured_check.py folds comb, equal_paths, star_max_hub and desc_path
(tests/structured_streams.py, capacity 2^20 + 3) window by window and through fold_windows, every
window's checksum and the final dense labels against the C oracle: with no GSGPU_* variable (the
production configuration), with the ring fold forced (GSGPU_FOLD_MODE=ring) and with the ring fold
and its warm set from 2^20 ids (GSGPU_RING_MIN_BITS=20). In the two ring environments the script
counts GS_K_RING launches; `comb` must have at least one, so a configuration that never reached
k_fold_ring fails. The streams and the oracle's results are written once (the `reference` fixture).
"""
import json
import os
import subprocess
import sys

import pytest

import structured_check

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "structured_check.py")

ENVS = {
    "production": {},
    "ring_forced": {"GSGPU_FOLD_MODE": "ring"},
    "ring_warm_from_2^20": {"GSGPU_RING_MIN_BITS": "20"},
}


def _env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSGPU_")}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def reference(tmp_path_factory, _oracle_built):
    path = str(tmp_path_factory.mktemp("structured") / "ref.npz")
    structured_check.make_ref(path)
    return path


@pytest.mark.parametrize("name", list(ENVS))
def test_structured_streams_per_environment(reference, name):
    p = subprocess.run([sys.executable, CHECK, "--ref", reference], env=_env(ENVS[name]), timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    r = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1])
    print(json.dumps(r["cases"]))
    bad = [c for c in r["cases"] if not c["ok"]]
    assert r["ok"] and not bad and [c["case"] for c in r["cases"]] == list(structured_check.CASES), bad
    assert r["ring_expected"] == bool(ENVS[name])
    if ENVS[name]:
        comb = [c for c in r["cases"] if c["case"] == "comb"][0]
        assert comb["ring_launches"] >= 1, comb
