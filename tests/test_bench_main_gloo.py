"""bench.py's main() itself -- argument handling, scene replication, stripe split, ray counting, the timing protocol
(barrier, MAX over ranks), verification against the oracle, the JSON line -- on CPU under gloo, world size 2, with a
stand-in for hiplib.HipContext that renders with the CPU oracle (test infrastructure; the product path has no such
fallback).  What the GPU tests cannot cover on a one-GPU box: main() with more than one rank."""
import ctypes
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_framering_gloo import OracleStripeRenderer   # noqa: E402


class StubContext(OracleStripeRenderer):
    """The calls bench.main() makes on a HipContext, answered by the oracle."""

    def __init__(self, local_rank):
        super().__init__(None, 0, 0, None)
        self.own = {}

    def build_from_heightmap(self, hmap, mmap):
        import svo_raytracer_amd.scene as scene
        self.pool = scene.build_scene(hmap.shape[0])[0]
        return int(self.pool.size)

    def pool_download(self, nbytes):
        return self.pool[:nbytes].copy()

    def pool_upload_device(self, ptr, nbytes):
        self.pool = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(ptr)).copy()

    def resize(self, w, h):
        self.w, self.h = w, h
        self.stripes = (0, 1, (h + 7) // 8, 0)

    def set_camera(self, cam):
        self.cam = cam

    def set_pipeline(self, p): pass
    def set_tuning(self, w, t): pass
    def set_hit_records(self, on): pass
    def set_reserved_cus(self, n): pass
    def set_batch(self, n, stride): pass
    def close(self): pass

    def count_frame(self):
        from oracle import oracle
        frame, mode, bounces, mirror, spp = self.params
        first, step, n, _ = self.stripes
        tot = dict(rays=0, iterations=0, alg_bytes=0, pixels=0, nan_rays=0)
        for j in range(n):
            y0 = (first + j * step) * 8
            if y0 >= self.h:
                continue
            st = oracle.render(self.pool, self.w, self.h, self.cam, frame, mode, bounces=bounces, mirror_mask=mirror, spp=spp,
                               rows=(y0, min(self.h, y0 + 8)), want_hits=False)["stats"]
            for k in tot:
                tot[k] += st.get(k, 0)
        return tot

    def time_frames(self, warm, iters):
        return np.full(iters, 1.0, np.float32)

    # library-owned slots (FrameRing uses them with one rank)
    def ring_create(self, slots, frames_per_slot, want_hits):
        super().ring_create(slots, frames_per_slot, want_hits)
        n = self.w * self.h
        self.own = {b: (np.zeros(frames_per_slot * n, np.uint32), np.zeros(frames_per_slot * n, np.float32)) for b in range(slots)}
        for b, (c, d) in self.own.items():
            self.slots[b] = (c.ctypes.data, d.ctypes.data, None, n)

    def ring_read(self, slot, k, want_hits=False):
        c, d = self.own[slot]
        n = self.w * self.h
        return {"rgba": c[k * n:(k + 1) * n].view(np.uint8).reshape(self.h, self.w, 4).copy(),
                "depth": d[k * n:(k + 1) * n].reshape(self.h, self.w).copy()}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, argv, out_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    import bench
    rc, line = bench.main(argv, ctx_factory=StubContext)
    assert rc == 0
    if rank == 0:
        json.dump(line, open(out_path, "w"))
    if dist.is_initialized():
        dist.destroy_process_group()


ARGS = ["--size", "64", "--width", "72", "--height", "50", "--steps", "5", "--warmup", "2", "--inflight", "2", "--batch", "2",
        "--full", "--cpu-seconds", "0", "--long-steps", "6"]


@pytest.mark.parametrize("world,scaling", [(2, "strong"), (2, "weak"), (3, "strong")])
def test_bench_main_under_gloo(tmp_path, world, scaling):
    out = str(tmp_path / "line.json")
    argv = ARGS + ["--gpus", str(world), "--scaling", scaling]
    mp.spawn(_worker, args=(world, _free_port(), argv, out), nprocs=world, join=True)
    line = json.load(open(out))
    assert line["verified"] is True and line["n_gpus"] == world and line["ranks_seen"] == world
    assert line["steps"] == 5 and line["warmup"] == 2 and line["frames_in_flight"] == 4
    assert line["rank_ms_per_step"]["min"] <= line["rank_ms_per_step"]["max"] and abs(line["ms_per_step"] - line["rank_ms_per_step"]["max"]) < 1e-3
    # rays: every rank counted its own stripes; the sum is the whole frame's
    from oracle import oracle
    import svo_raytracer_amd.scene as scene
    from svo_raytracer_amd.cameras import CAMERAS
    pool = scene.build_scene(64)[0]
    h = 50 * world if scaling == "weak" else 50
    want = [oracle.render(pool, 72, h, CAMERAS["K1"], f, 0, want_hits=False)["stats"]["rays"] for f in (4, 8)]
    assert line["config"]["rays_per_frame"] == int(round(sum(want) / 2.0))
    assert line["value"] > 0 and line["unit"] == "Mrays/s" and line["scaling"] == scaling
    # the second, longer timed region of an N > 1 run, as an extra key
    assert line["value_long_run"] > 0 and line["long_run_steps"] == 6 and line["driver"].startswith("torch.distributed")


def test_bench_main_camera_path_under_gloo(tmp_path):
    """--camera-path orbit at world size 2: every frame with its own camera and frameNumber 1, verified per frame"""
    out = str(tmp_path / "line.json")
    argv = ARGS + ["--gpus", "2", "--camera-path", "orbit"]
    mp.spawn(_worker, args=(2, _free_port(), argv, out), nprocs=2, join=True)
    line = json.load(open(out))
    assert line["verified"] is True and "its own camera" in line["config"]["verification"]
    assert "moving along path" in line["config"]["workload"] and line["value"] > 0


def test_bench_main_one_rank_stub(tmp_path):
    """one rank, no launcher: library-owned slots, frames read back through the ring"""
    out = str(tmp_path / "line.json")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        os.environ.pop(k, None)
    import bench
    rc, line = bench.main(ARGS + ["--gpus", "1"], ctx_factory=StubContext)
    assert rc == 0 and line["verified"] is True and line["ranks_seen"] == 1 and line["gather_ms"] is None
    # (value_one_frame_at_a_time is the wall clock of the reference's loop through JNI-typed calls: GPU only)
    assert line["kernel_rate_isolated"] > 0 and line["value_one_frame_at_a_time"] is None and line["comm_cus_per_xcd"] == 0


PLAIN = ["--size", "64", "--width", "72", "--height", "50", "--steps", "5", "--warmup", "2", "--inflight", "2", "--batch", "2", "--gpus", "1"]


def test_bench_plain_run_is_the_headline_alone_and_dumps_its_last_frame(tmp_path):
    """without --full: no leg behind the headline runs (no check against the oracle, no longer region, no isolated frames, no
    CPU baseline), the line still carries the headline's keys; --dump-outputs writes the frame of the LAST timed step
    (frameNumber 2 + warm-up + steps - 1) as float32 arrays, the same bytes on every run"""
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        os.environ.pop(k, None)
    import bench
    from oracle import oracle
    import svo_raytracer_amd.scene as scene
    from svo_raytracer_amd.cameras import CAMERAS
    dumps = []
    for d in ("a", "b"):
        rc, line = bench.main(PLAIN + ["--dump-outputs", str(tmp_path / d)], ctx_factory=StubContext)
        assert rc == 0 and line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
        assert (line["unit"], line["higher_is_better"], line["dtype"]) == ("Mrays/s", True, "f32") and line["metric"].startswith("Mrays/s")
        assert line["verified"] is None and line["config"]["verification"] is None and line["cpu_baseline"] is None
        assert line["value_long_run"] is None and line["kernel_rate_isolated"] is None and line["roofline"]["kernel_ms_isolated"] is None
        assert line["moving_camera"] is None and line["default_abi"] is None and line["reference_loop"] is None and line["by_camera"] is None
        assert sorted(os.listdir(tmp_path / d)) == ["depth.npy", "rgba.npy"]
        dumps.append({k: np.load(tmp_path / d / (k + ".npy")) for k in ("rgba", "depth")})
    ref = oracle.render(scene.build_scene(64)[0], 72, 50, CAMERAS["K1"], 2 + 2 + 5 - 1, 0, want_hits=False)
    for z in dumps:
        assert z["rgba"].dtype == np.float32 and z["rgba"].shape == (50, 72, 4) and (z["rgba"] == ref["rgba"]).all()
        assert z["depth"].dtype == np.float32 and z["depth"].shape == (50, 72)
        assert (z["depth"].view(np.uint32) == ref["depth"].view(np.uint32)).all()
    assert all(dumps[0][k].tobytes() == dumps[1][k].tobytes() for k in dumps[0])


def test_a_leg_named_by_its_own_option_runs_without_full_and_full_sets_the_defaults():
    import bench
    a = bench.parse([])
    assert (a.full, a.verify, a.long_steps, a.moving, a.default_abi, a.ref_loop, a.by_camera, a.isolated, a.cpu_seconds) == (False, 0, 0, 0, 0, 0, 0, 0, 0)
    a = bench.parse(["--full"])
    assert (a.verify, a.long_steps, a.moving, a.default_abi, a.ref_loop, a.by_camera, a.isolated, a.cpu_seconds) == (1, 400, 1, 1, 1, 1, 1, 15.0)
    a = bench.parse(["--verify", "1", "--long-steps", "7"])
    assert (a.verify, a.long_steps, a.moving, a.cpu_seconds) == (1, 7, 0, 0)
    a = bench.parse(["--full", "--verify", "0", "--default-abi", "0"])
    assert (a.verify, a.default_abi, a.ref_loop, a.by_camera, a.moving) == (0, 0, 0, 0, 1)


def test_dump_outputs_samples_a_frame_that_does_not_fit(tmp_path, monkeypatch):
    """a frame larger than the limit is cut to a seeded sample of pixels: the same pixels every time, their indices written
    next to them, everything together within the limit; hit records go out as float64 (a pointer does not fit a float32)"""
    import torch
    import bench
    h, w = 37, 53
    rng = np.random.default_rng(5)
    col = rng.integers(-2 ** 31, 2 ** 31, size=(h, w), dtype=np.int64).astype(np.int32)
    dep = rng.random((h, w), dtype=np.float32)
    hits = rng.integers(0, 2 ** 31, size=(h, w, 4), dtype=np.int64).astype(np.int32)
    images = (9, torch.from_numpy(col), torch.from_numpy(dep), torch.from_numpy(hits))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40000)      # the whole frame would take 37 * 53 * 52 = 101 972 bytes
    out = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), images)
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["depth.npy", "hits.npy", "pixel_index.npy", "rgba.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= 40000
        out.append({f[:-4]: np.load(tmp_path / d / f) for f in files})
    z = out[0]
    idx = z["pixel_index"].astype(np.int64)
    assert z["pixel_index"].dtype == np.float64 and 500 < idx.size < h * w and (np.diff(idx) > 0).all() and idx[-1] < h * w
    assert z["rgba"].dtype == np.float32 and (z["rgba"] == col.view(np.uint8).reshape(h * w, 4)[idx]).all()
    assert z["depth"].dtype == np.float32 and (z["depth"] == dep.reshape(-1)[idx]).all()
    assert z["hits"].dtype == np.float64 and (z["hits"] == hits.reshape(h * w, 4)[idx]).all()
    assert all(out[0][k].tobytes() == out[1][k].tobytes() for k in z)
