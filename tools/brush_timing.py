"""The reference's own brush strokes (Main.placeSDF: Sphere(r = 64); Main.java:244-249: Box(10, 20, 30)) with world_size
8196 and max_lod 13 on the 8192^3 bench scene, at the K0 camera's crosshair pick (its centre ray sees sky, so the pick is the eye, on the world's edge) and on the terrain
below it.  Three figures per stroke:
  gpu_ms    svo_brush_sphere / svo_brush_box on the device pool (svo_brush_info: planning + writing, without the table)
  cpu_ms    the restatement of Octree.useSDFBrush (oracle/octree_restatement.cpp) on a host copy of the same pool
  route_ms  today's route: the restatement + the two svo_pool_update calls (wall)
and the wall time of the GPU call (with the descriptor table following).  Then svo_pool_compact on what the strokes left:
lengths before and after, GPU and wall time, records and levels (svo_compact_info).  A measurement script (it loads the oracle-side
restatement), not product code.  --md FILE writes the table as markdown."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import svo_raytracer_amd.scene as scene
from svo_raytracer_amd import hiplib, hostlib
from svo_raytracer_amd.cameras import CAMERAS
from oracle import octree as restated

N, WORLD, LOD = 8192, 8196, 13
STROKES = [("sphere", 64, 0), ("sphere", 64, 2), ("box", (10, 20, 30), 0), ("box", (10, 20, 30), 2)]


def crosshair(ctx, h):
    """the voxel the centre pixel of K0 sees: the eye plus depth along the centre ray (Main.java:139-146), on the terrain"""
    cam = np.asarray(CAMERAS["K0"], dtype=np.float32).reshape(5, 3)
    ctx.render(None, 1920, 1080, cam, 2, 0)
    _, depth, _ = ctx.read_pixel(960, 540)
    d = cam[1:].sum(axis=0)
    d = d / np.linalg.norm(d)
    p = (cam[0] + d * depth - 1.0) * WORLD       # Camera.getRayPickLocation (Camera.java:31-34): depth 0 (sky) = the eye
    pick = tuple(int(v) for v in p)
    x, z = int(np.clip(p[0], 200, N - 200)), int(np.clip(p[2], 200, N - 200))
    return pick, (x, int(h[z, x]), z), float(depth)


def compact_leg(gpu):
    """svo_pool_compact on the pool the strokes left, and once more on its own result (which must come back as it is); the K0
    frame before and after must agree in everything but the hit records' pointers"""
    cam = CAMERAS["K0"]
    before = gpu.render(None, 1920, 1080, cam, 2, 0)
    out = ["| call | bytes before | bytes after | gpu_ms | call wall ms | records | levels |", "|---|---|---|---|---|---|---|"]
    for call in ("after the strokes", "again"):
        t0 = time.perf_counter()
        old, new = gpu.pool_compact()
        wall_ms = (time.perf_counter() - t0) * 1e3
        info = gpu.compact_info()
        out.append("| %s | %d | %d | %.3f | %.3f | %d | %d |" % (call, old, new, info["gpu_ms"], wall_ms, info["records"], info["levels"]))
    after = gpu.render(None, 1920, 1080, cam, 2, 0)
    same = (before["rgba"] == after["rgba"]).all() and (before["depth"].view(np.uint32) == after["depth"].view(np.uint32)).all() and all(
        (before["hits"][k] == after["hits"][k]).all() for k in ("value", "raw_normal", "level", "iter"))
    out += ["", "K0 frame (1920x1080, mode 0) equal before and after but for the pointers: %s; pixels whose pointer moved: %d" % (
        bool(same), int((before["hits"]["pointer"] != after["hits"]["pointer"]).sum()))]
    return out


def main():
    md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
    h, m = scene.scene_maps(N)
    gpu, route = hiplib.HipContext(0), hiplib.HipContext(0)
    nb = gpu.build_from_heightmap(h, m)
    pool = gpu.pool_download(nb)
    route.pool_upload(pool)
    gpu.set_pipeline(1); route.set_pipeline(1)
    pick, ground, depth = crosshair(gpu, h)
    gpu.derived_info(); route.derived_info()
    o = hostlib.Octree((nb + (256 << 20)) // 1024)
    o.adopt(pool)
    rows = []
    for where, org, (kind, size, val) in [(w, o_, s_) for w, o_ in (("pick", pick), ("terrain", ground)) for s_ in STROKES]:
        t0 = time.perf_counter()
        if kind == "sphere":
            cb = restated.useSDFBrushSphere(o, org, size, val, worldSize=WORLD, maxLOD=LOD)
        else:
            cb = restated.useSDFBrushBox(o, org, size[0], size[1], size[2], val, worldSize=WORLD, maxLOD=LOD)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        host = o.getByteBuffer()
        t1 = time.perf_counter()
        for s, e in ((cb[0], cb[1]), (cb[2], cb[3])):
            if e > s:
                route.pool_update(host, s, e)
        route_ms = cpu_ms + (time.perf_counter() - t1) * 1e3
        t2 = time.perf_counter()
        got = gpu.brush_sphere(org, size, val, WORLD, LOD) if kind == "sphere" else gpu.brush_box(org, *size, val, WORLD, LOD)
        wall_ms = (time.perf_counter() - t2) * 1e3
        info = gpu.brush_info()
        same = got == cb and np.array_equal(gpu.pool_download(cb[3]), host)
        rows.append((where, org, kind, size, val, info["gpu_ms"], cpu_ms, route_ms, wall_ms, info["visited"], info["subdivided"], cb[3] - cb[2], same))
    lines = ["K0 crosshair depth %.4f: pick %s, terrain below it %s; world_size %d, max_lod %d, pool %d bytes" % (depth, pick, ground, WORLD, LOD, nb), "",
             "| where | origin | stroke | value | gpu_ms | cpu_ms (restatement) | route_ms (restatement + 2 updates) | GPU call wall ms | visited | subdivided | appended bytes | bytes equal |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %s %s | %d | %.3f | %.3f | %.3f | %.3f | %d | %d | %d | %s |" % r)
    lines += ["", "svo_pool_compact after these strokes:", ""] + compact_leg(gpu)
    print("\n".join(lines))
    if md:
        open(md, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
