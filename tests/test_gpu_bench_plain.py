"""A plain bench.py run on the GPU -- no --full -- is the headline region alone, and --dump-outputs writes the frame its last
timed step rendered: bit for bit the oracle's frame, from inside the throughput configuration (launches in flight, batches,
a partial last batch)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_timed_frame(tmp_path):
    from oracle import oracle
    import svo_raytracer_amd.scene as scene
    from svo_raytracer_amd.cameras import CAMERAS
    w, h, steps, warm = 328, 203, 11, 3      # 11 steps in batches of 4: the last submission is a partial one (3 frames)
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warm),
                        "--size", "128", "--width", str(w), "--height", str(h), "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == steps and line["warmup"] == warm and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["verified"] is None and line["value_long_run"] is None and line["default_abi"] is None and line["cpu_baseline"] is None
    assert line["reference_loop"] is None and line["moving_camera"] is None and line["roofline"]["kernel_ms_isolated"] is None
    ref = oracle.render(scene.build_scene(128)[0], w, h, CAMERAS["K1"], 2 + warm + steps - 1, 0, want_hits=False)
    rgba, depth = np.load(out / "rgba.npy"), np.load(out / "depth.npy")
    assert rgba.dtype == np.float32 and rgba.shape == (h, w, 4) and (rgba == ref["rgba"]).all()
    assert depth.dtype == np.float32 and (depth.view(np.uint32) == ref["depth"].view(np.uint32)).all()
