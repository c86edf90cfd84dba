"""More than one rank on the GPU box: the box has ONE MI355X and RCCL refuses two ranks on one device, but the copy
exchange (svo_ring_forward_slot: device-to-device copies into the frame owner's buffer through its IPC handle) and gloo
(control messages only) do not.  Two and three processes, each with its own HipContext on GPU 0: pool replication,
stripe split, forwarding with sequence words, reassembly on rank 0 -- the whole N > 1 data path on real hardware except
the xGMI hop itself -- against the oracle; then bench.py itself run that way."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, w, h, nbuf, batch, steps, want_hits, out_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import svo_raytracer_amd.scene as scene
    from svo_raytracer_amd import hiplib
    from svo_raytracer_amd.cameras import CAMERAS
    from svo_raytracer_amd.framering import FrameRing, replicate_pool
    pool = scene.build_scene(128)[0] if rank == 0 else None
    dpool = replicate_pool(dist, pool, rank, world, device="cpu")
    ctx = hiplib.HipContext(0)
    ctx.pool_upload(dpool.numpy())
    ctx.resize(w, h)
    ctx.set_camera(CAMERAS["K1"])
    ctx.set_pipeline(1)
    ctx.set_tuning(6, 9)
    ring = FrameRing(ctx, w, h, world=world, rank=rank, nbuf=nbuf, device="cuda", dist=dist, want_hits=want_hits,
                     first_frame=2, params=dict(render_mode=0, buffer_end=int(dpool.numel())), batch=batch, exchange="copy")
    left = steps
    while left > 0:
        n = min(batch, left)
        ring.step(n)
        left -= n
    torch.cuda.synchronize()
    dist.barrier()          # every rank's copies have been enqueued and completed on its streams
    ring.drain()
    if rank == 0:
        out, i = {}, 0
        for b in range(nbuf):
            for k in range(ring.count_of[b]):
                imgs = ring.frame_images(b, k)
                out["frame%d" % i] = np.int64(imgs[0])
                out["color%d" % i] = imgs[1].numpy()
                out["depth%d" % i] = imgs[2].numpy()
                if want_hits:
                    out["hits%d" % i] = imgs[3].numpy()
                i += 1
        out["nframes"] = np.int64(i)
        np.savez(out_path, **out)
    dist.barrier()
    ctx.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,nbuf,batch,steps,want_hits", [(2, 2, 1, 5, False), (2, 3, 2, 9, True), (3, 2, 3, 8, False)])
def test_copy_exchange_between_ranks_on_one_gpu(tmp_path, world, nbuf, batch, steps, want_hits):
    import svo_raytracer_amd.scene as scene
    from oracle import oracle
    from svo_raytracer_amd import hiplib
    from svo_raytracer_amd.cameras import CAMERAS
    w, h = 200, 120
    out = str(tmp_path / "frames.npz")
    mp.spawn(_worker, args=(world, _free_port(), w, h, nbuf, batch, steps, want_hits, out), nprocs=world, join=True)
    z = np.load(out)
    pool = scene.build_scene(128)[0]
    assert int(z["nframes"]) >= 1
    seen = set()
    for i in range(int(z["nframes"])):
        fr = int(z["frame%d" % i])
        seen.add(fr)
        ref = oracle.render(pool, w, h, CAMERAS["K1"], fr, 0, want_hits=want_hits)
        assert (z["color%d" % i].view(np.uint8).reshape(h, w, 4) == ref["rgba"]).all(), fr
        assert (z["depth%d" % i].view(np.uint32) == ref["depth"].view(np.uint32)).all(), fr
        if want_hits:
            assert z["hits%d" % i].astype(np.int32).tobytes() == ref["hits"].view(np.int32).reshape(h, w, 4).tobytes(), fr
    assert max(seen) == 2 + steps - 1       # the last frame dispatched is among those the ring still holds


def test_bench_two_ranks_on_one_gpu_copy_exchange():
    """bench.py --gpus 2 --exchange copy with both ranks on GPU 0 (gloo for the control plane): verified line"""
    env = dict(os.environ, SVO_BENCH_BACKEND="gloo", SVO_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--exchange", "copy", "--size", "512",
           "--width", "640", "--height", "360", "--steps", "12", "--warmup", "4", "--inflight", "2", "--batch", "2", "--waves", "6",
           "--full", "--cpu-seconds", "0", "--isolated", "0"]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["verified"] is True and line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["exchange"] == "copy"
    assert line["value"] > 0


def _bench_line(cmd, env=None, timeout=900):
    p = subprocess.run(cmd, env=env or dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def test_one_rank_under_the_launcher_reproduces_the_plain_run():
    """the driver starts N > 1 as `python -m torch.distributed.run ... bench.py --gpus N`; at N = 1 under that launcher the line
    must be the plain `bench.py --gpus 1` line: same workload, same ray count, verified, the value within a box's spread of a
    20-step region (both are all start and drain)"""
    common = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--cpu-seconds", "0", "--moving", "0", "--long-steps", "200"]
    plain = _bench_line([sys.executable, os.path.join(ROOT, "bench.py")] + common)
    under = _bench_line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                         "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py")] + common)
    for ln in (plain, under):
        assert ln["verified"] is True and ln["n_gpus"] == 1 and ln["steps"] == 20 and ln["fallback_from"] == []
        # the 11 ms region is bracketed by a longer one on the same line, and by the run through JNI-typed calls with no
        # tuning call at all: the library's defaults are the benchmarked configuration
        assert ln["long_run_steps"] == 200 and 0.8 < ln["value_long_run"] / ln["value"] < 1.35
        d = ln["default_abi"]
        assert d["verified"] is True and d["launch_shape"] == {"persistent_waves": 2560, "waves_per_cu": 10, "slots": 6, "frames_per_slot": 4}
        assert 0.85 < d["value"] / ln["value"] < 1.18 and 0.92 < d["value_long_run"] / ln["value_long_run"] < 1.08, (d, ln["value"], ln["value_long_run"])
    assert plain["config"]["rays_per_frame"] == under["config"]["rays_per_frame"]
    assert plain["config"]["workload"] == under["config"]["workload"]
    assert 0.8 < under["value"] / plain["value"] < 1.25, (plain["value"], under["value"])


@pytest.mark.parametrize("n", [2, 3])
def test_bench_group_driver_on_one_gpu(n):
    """bench.py --gpus N --driver group: ONE process, the N members behind the C ABI (svo_group_*), here all on GPU 0;
    the line carries the second, longer timed region of an N > 1 run"""
    env = dict(os.environ, SVO_BENCH_ONE_GPU="1")
    line = _bench_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--driver", "group", "--exchange", "copy",
                        "--size", "512", "--width", "640", "--height", "360", "--steps", "12", "--warmup", "4", "--inflight", "3",
                        "--batch", "2", "--waves", "6", "--full", "--long-steps", "24", "--cpu-seconds", "0"], env=env)
    assert line["verified"] is True and line["n_gpus"] == n and line["driver"].startswith("group")
    assert line["value"] > 0 and line["value_long_run"] > 0 and line["long_run_steps"] == 24
    assert "svo_group_" in line["config"]["workload"]


# ---- BASELINE configs 4 and 5 through the torch driver's split (two ranks sharing the GPU, copy exchange), against the
# reference shader's own images
def _worker_config(rank, world, port, cfg, out_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import svo_raytracer_amd.scene as scene
    from svo_raytracer_amd import hiplib
    from svo_raytracer_amd.framering import FrameRing, replicate_pool
    pool = scene.build_scene(cfg["size"])[0] if rank == 0 else None
    dpool = replicate_pool(dist, pool, rank, world, device="cpu")
    ctx = hiplib.HipContext(0)
    ctx.pool_upload(dpool.numpy())
    w, h = cfg["w"], cfg["h"]
    ctx.resize(w, h)
    ctx.set_camera(np.asarray(cfg["cam"], dtype=np.float32))
    seq = cfg.get("seq", 1)
    if seq > 1:
        ctx.set_progressive(True)
        ctx.set_sequence(seq, True)
    ring = FrameRing(ctx, w, h, world=world, rank=rank, nbuf=2, device="cuda", dist=dist, want_hits=cfg["hits"],
                     first_frame=cfg["frame"], batch=1, exchange="copy", advance=seq == 1,
                     params=dict(render_mode=cfg["mode"], buffer_end=int(dpool.numel()), bounces=cfg["bounces"], mirror_mask=cfg["mirror"]))
    ring.step(1)
    torch.cuda.synchronize()
    dist.barrier()
    ring.drain()
    if rank == 0:
        imgs = ring.frame_images(0, 0)
        out = {"color": imgs[1].numpy(), "depth": imgs[2].numpy()}
        if cfg["hits"]:
            out["hits"] = imgs[3].numpy()
        np.savez(out_path, **out)
    dist.barrier()
    ctx.close()
    dist.destroy_process_group()


def test_config4_through_two_ranks_equals_the_reference_shader(tmp_path):
    from svo_raytracer_amd import hiplib
    from test_config3 import GOLD, _check, _meta
    z = np.load(GOLD)
    w, h, frame, mode, bounces, mirror = _meta(z, "c4_f2")
    cfg = dict(size=8192, w=w, h=h, frame=frame, mode=mode, bounces=bounces, mirror=mirror, hits=True, cam=z["c4_f2/cam"].tolist())
    out = str(tmp_path / "c4.npz")
    mp.spawn(_worker_config, args=(2, _free_port(), cfg, out), nprocs=2, join=True)
    r = np.load(out)
    res = {"rgba": r["color"].view(np.uint8).reshape(h, w, 4), "depth": r["depth"],
           "hits": np.ascontiguousarray(r["hits"].astype(np.int32)).reshape(-1, 4).view(hiplib.HIT_DTYPE).reshape(h, w)}
    _check(res, z, "c4_f2", int(z["step"][0]))


def test_config5_through_two_ranks_equals_the_reference_shader(tmp_path):
    z = np.load(os.path.join(ROOT, "tests", "golden", "c5_progressive.npz"))
    n, w, h, mode = (int(v) for v in z["meta"])
    st = int(z["step"][0])
    cfg = dict(size=n, w=w, h=h, frame=2, mode=mode, bounces=2, mirror=0, hits=False, cam=z["cam"].tolist(), seq=64)
    out = str(tmp_path / "c5.npz")
    mp.spawn(_worker_config, args=(2, _free_port(), cfg, out), nprocs=2, join=True)
    r = np.load(out)
    rgba = r["color"].view(np.uint8).reshape(h, w, 4)
    assert np.array_equal(rgba[::st, ::st], z["f65/rgba"])
    assert np.array_equal(r["depth"].view(np.uint32)[::st, ::st], z["f65/depth_bits"])


def test_ranks_under_the_launcher_negotiate_the_exchange_before_they_touch_the_gpu():
    """How the round driver starts N > 1: `python -m torch.distributed.run ... bench.py --gpus N` with the default exchange.  Here
    both ranks share GPU 0, where RCCL cannot make its communicator -- the situation a first contact with a node may produce for
    other reasons: every rank's probe child fails (or is killed at its time limit), the ranks agree over gloo, and the run
    itself goes through the copy exchange and says on its line what it tried (bench.negotiate_exchange)."""
    env = dict(os.environ, SVO_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("SVO_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--size", "512", "--width", "640",
           "--height", "360", "--steps", "12", "--warmup", "4", "--inflight", "2", "--batch", "2", "--full", "--cpu-seconds", "0", "--isolated", "0",
           "--long-steps", "24", "--probe-timeout", "150"]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["verified"] is True and line["n_gpus"] == 2 and line["ranks_seen"] == 2
    assert line["exchange"] == "copy" and [f["exchange"] for f in line["fallback_from"]] == ["rccl"], line["fallback_from"]
    assert line["fallback_from"][0]["failed"].startswith("probe: ") and line["value"] > 0 and line["value_long_run"] > 0
