"""svo_cast_rays_device next to the frame kernel on the same rays: the primary rays of the benchmark frame (8192^3 scene,
1920x1080, camera K1) cast through the ray kernel (csrc/svo_rays.hip.h), and the same context's mode-0, bounces-1 frame,
whose only cast per pixel is that ray.  Both on the context's defaults (descriptor walk, automatic launch shape), after
warm-up; GPU time between HIP events around calls that follow one another on one stream (svo_time_frames; the caller's
stream and torch events for the casts), Mrays/s = 1920 * 1080 / time.  The frame also shades
the hit and stores colour and depth; the ray kernel loads 24 bytes per ray instead of forming the direction.  The records of
the two must be the same bytes: checked here too.  The rays are cast twice: in the caller's natural order, row by row, and in
the order the frame kernel takes its pixels in (8 x 8 tiles), which separates what the order of the rays costs from what the
kernel costs.  A measurement script, not product code.  --md FILE writes the table as
markdown; --n EDGE takes a smaller scene (a rehearsal, not the benchmark)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import svo_raytracer_amd.scene as scene
from svo_raytracer_amd import hiplib
from svo_raytracer_amd.cameras import CAMERAS

W, H, WARMUP, ITERS = 1920, 1080, 5, 30


def pixel_rays(cam, w, h):
    """the frame's primary rays as the shader forms them before normalising (svotrace.comp:662-675), in float32, unfused"""
    o, l1, l2, r1, r2 = np.asarray(cam, dtype=np.float32).reshape(5, 3)
    f = np.float32
    px = ((np.arange(w, dtype=np.float32) + f(0.5)) / f(w))[None, :, None]
    py = ((np.arange(h, dtype=np.float32) + f(0.5)) / f(h))[:, None, None]
    a, b = l1 + py * (l2 - l1), r1 + py * (r2 - r1)
    rays = np.empty((h, w, 6), dtype=np.float32)
    rays[..., :3] = o
    rays[..., 3:] = a + px * (b - a)
    return rays.reshape(-1, 6)


def stats(ms):
    ms = np.sort(np.asarray(ms, dtype=np.float64))
    return float(np.median(ms)), float(ms[0]), float(ms[-1])


def main():
    import torch
    md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
    n = int(sys.argv[sys.argv.index("--n") + 1]) if "--n" in sys.argv else 8192
    cam = CAMERAS["K1"]
    ctx = hiplib.HipContext(0)
    nb = ctx.build_from_heightmap(*scene.scene_maps(n))
    ctx.set_pipeline(1)
    info = ctx.derived_info()
    # the frame: one primary cast per pixel, nothing behind it
    ctx.resize(W, H)
    ctx.set_camera(cam)
    ctx.set_params(2, 0, 0, 0, 1, 0, 1)
    frame_ms = stats(ctx.time_frames(WARMUP, ITERS))
    frame_waves = ctx.launch_info()["waves"]
    frame_hits = ctx.read_hits().reshape(-1)
    # the same rays through the ray kernel, from and to device memory
    rays = pixel_rays(cam, W, H)
    # ... in the caller's order (row by row: a wave's 64 rays are a 64 x 1 strip), and in the order the frame kernel takes its
    # pixels in (8 x 8 tiles: a wave's 64 rays are one tile)
    idx = np.arange(W * H).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    want = frame_hits.view(np.uint32).reshape(-1, 4)
    cast_ms, same = {}, True
    for order, perm in (("rows", None), ("tiles", idx)):
        r = rays if perm is None else np.ascontiguousarray(rays[perm])
        d_rays = torch.from_numpy(r).cuda()
        d_hits = torch.zeros((r.shape[0], 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        # as svo_time_frames times the frames: the calls back to back on one stream, an event between two of them
        stream = torch.cuda.Stream()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(ITERS + 1)]
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            for k in range(WARMUP):
                ctx.cast_rays_device(d_rays.data_ptr(), r.shape[0], d_hits.data_ptr())
            ev[0].record()
            for k in range(ITERS):
                ctx.cast_rays_device(d_rays.data_ptr(), r.shape[0], d_hits.data_ptr())
                ev[k + 1].record()
            stream.synchronize()
        ctx.set_stream(None)
        cast_ms[order] = stats([ev[k].elapsed_time(ev[k + 1]) for k in range(ITERS)])
        # ... and one call alone on an idle GPU, as a host makes it (svo_cast_info)
        ctx.cast_rays_device(d_rays.data_ptr(), r.shape[0], d_hits.data_ptr())
        ctx.sync()
        alone_ms = ctx.cast_info()["gpu_ms"]
        same = same and bool((d_hits.cpu().numpy().view(np.uint32) == (want if perm is None else want[perm])).all())
    cinfo = ctx.cast_info()
    hit_share = float((frame_hits["pointer"] != 0).mean())
    mrays = lambda t: W * H / t / 1e3
    lines = ["%d^3 scene (pool %d bytes, %d descriptors, walkable %s), %dx%d, camera K1, %.1f %% of the rays hit; %d timed "
             "calls each after %d warm-up calls" % (n, nb, info["descriptors"], info["walkable"], W, H, 100 * hit_share, ITERS, WARMUP), "",
             "| kernel | waves | walk | median ms | min ms | max ms | Mrays/s (median) |", "|---|---|---|---|---|---|---|",
             "| frame kernel, mode 0, bounces 1 (svo_time_frames) | %d | %d | %.4f | %.4f | %.4f | %.1f |" % (
                 frame_waves, 1 if info["walkable"] else 0, frame_ms[0], frame_ms[1], frame_ms[2], mrays(frame_ms[0])),
             ] + ["| svo_cast_rays_device, rays in %s (events between back-to-back calls) | %d | %d | %.4f | %.4f | %.4f | %.1f |" % (
                 what, cinfo["waves"], cinfo["walk"], cast_ms[o][0], cast_ms[o][1], cast_ms[o][2], mrays(cast_ms[o][0]))
                 for o, what in (("rows", "row order"), ("tiles", "8 x 8 tile order"))] + ["",
             "ray kernel / frame kernel (median time): %.3f in row order, %.3f in tile order; hit records byte-equal: %s" % (
                 cast_ms["rows"][0] / frame_ms[0], cast_ms["tiles"][0] / frame_ms[0], same),
             "one call alone on an idle GPU, host waiting (svo_cast_info's gpu_ms, tile order): %.4f ms" % alone_ms]
    print("\n".join(lines))
    if md:
        open(md, "w").write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
