"""bench.py's plain run: the result line of a short stream, nothing of the --full legs in it,
and --dump-outputs' arrays (float32 / float64 .npy of the last timed step, under 64 MB)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 12


@pytest.mark.gpu
def test_plain_run_result_line_and_dump(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--frames", str(FRAMES), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["unit"] == "frames/s" and r["higher_is_better"] is True and r["dtype"] == "u8"
    assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0
    # value is frames over the timed steps' time
    assert r["value"] == pytest.approx(FRAMES / (r["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("cpu_baseline", "parity", "roofline", "searches", "pose_optimization", "bag_of_words",
              "dropin_per_frame", "chained_per_frame"):
        assert k not in r, k
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(out / "*.npy"))}
    assert {"keypoint_count", "match_count", "line_count", "keypoints", "descriptors", "matches", "lines", "gray",
            "assoc_detections", "object_ints", "object_floats", "sample_frames"} <= set(arrays)
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert not any(np.isnan(a).any() for a in arrays.values())
    cnt, sel = arrays["keypoint_count"], arrays["sample_frames"].astype(int)
    assert cnt.shape == (FRAMES,) and cnt.min() > 0 and r["mean_keypoints"] == pytest.approx(cnt.mean(), rel=1e-6)
    kp = arrays["keypoints"]
    assert kp.shape[0] == len(sel) and kp.shape[2] == 7
    for i, t in enumerate(sel):  # rows up to the count hold keypoints inside the image, rows past it are zero
        n = int(cnt[t])
        assert (kp[i, :n, 0] >= 0).all() and (kp[i, :n, 0] < 640).all() and (kp[i, :n, 2] > 0).all()
        assert not kp[i, n:].any() and not arrays["descriptors"][i, n:].any()
