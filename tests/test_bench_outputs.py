"""bench.py --dump-outputs: the hypothesis list the last timed step computed, written as float64 arrays, is the oracle's
list for the same cloud bit for bit, and the result line reports the timed steps it was asked for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FIELDS = ("axis", "approach", "binormal", "bottom", "surface", "width", "sample", "orientation", "cam_source", "n_in_box",
          "half_antipodal", "full_antipodal", "svm_keep", "valid", "finger_index", "depth_index")


def test_dump_outputs_are_the_oracles_list(tmp_path):
    from agile_grasp_amd import synthetic
    from oracle import oracle_py as O

    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "small", "--steps", "3", "--warmup", "1",
                        "--spin-seconds", "0", "--no-cpu-baseline", "--dump-outputs", str(out)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(line["config"]["hypotheses"])

    sc = synthetic.config("small")
    ref = O.find_hands(O.default_params(sc.cam_origins), sc.xyz, sc.cam, sc.samples)["hyps"]
    assert len(ref) > 10 and line["config"]["hypotheses"] == len(ref)
    assert sorted(os.listdir(out)) == sorted(f"hyp_{f}.npy" for f in FIELDS)
    for f in FIELDS:
        got = np.load(out / f"hyp_{f}.npy")
        assert got.dtype == np.float64 and got.shape == ref[f].shape, f
        assert np.array_equal(got, ref[f].astype(np.float64)), f
