"""bench.py's SURVEY.md 8(f) lines end to end at small sizes: edge-file ingestion parses the text of
a generated stream back into exactly its ids (and the C oracle parses the same text), and
BipartitenessCheck on a bipartite stream stays bipartite with the component counts of the CC path."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "1", "--warmup", "1"]
                                  + list(extra), timeout=300).decode()
    assert len(out.strip().splitlines()) == 1, out[:2000]
    return json.loads(out)


def test_bench_parse_line():
    line = _bench("--workload", "parse", "--scale", "16", "--edge-factor", "4")
    assert line["verify"] == {"lines": 4 << 16, "equal_to_generated_ids": True}
    assert "equal" in line["cpu_baseline"]["sample"] and line["cpu_baseline"]["value"] > 0
    assert 0 < line["roofline"]["frac"] <= 1 and line["value"] > 0


def test_plain_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) at a small size: the headline fields, none of the --full ones, and
    --dump-outputs writes the last timed step's emission: every label (the array is small enough to
    be whole), consistent with the line's counts and checksum."""
    import numpy as np
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                                   "--warmup", "1", "--scale", "16", "--window-log2", "14", "--dump-outputs",
                                   str(tmp_path / "o")], timeout=300).decode()
    assert len(out.strip().splitlines()) == 1, out[:2000]
    line = json.loads(out)
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "edges/s"
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - (16 << 16)) < 1e-3 * (16 << 16)
    assert "cpu_baseline" not in line and "final_checksum_vs_fixture" not in line
    assert "compress_share" not in line["kernels"]
    lab, s = np.load(tmp_path / "o" / "labels.npy"), np.load(tmp_path / "o" / "summary.npy")
    assert lab.dtype == np.float64 and lab.shape == (1 << 16,) and s.dtype == np.float64
    seen = lab >= 0
    assert int(seen.sum()) == line["final_vertices"] == int(s[0])
    assert len(np.unique(lab[seen])) == line["final_components"] == int(s[1])
    assert np.all(lab[seen] <= np.nonzero(seen)[0]) and np.all(lab[lab[seen].astype(np.int64)] == lab[seen])
    assert (int(s[2]) << 32) | int(s[3]) == int(line["final_checksum"])


def test_bench_bip_line():
    line = _bench("--workload", "bip", "--scale", "14", "--edge-factor", "8", "--window-log2", "12")
    v = line["verify"]
    assert v["bipartite"] is True and v["equal_to_cc_counts"] is True and v["vertices"] > 0
    assert line["cpu_baseline"]["value"] > 0 and 0 < line["roofline"]["frac"] <= 1
