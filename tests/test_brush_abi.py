"""CPU-side checks of the brush's boundary (svo_brush_sphere / svo_brush_box / svo_pool_download_range / svo_brush_info and
the group's strokes): declared in the header, listed by the binding, exported by the library with their JNI natives and
the Java twin's declarations, and a null context is refused, not dereferenced."""
import ctypes
import os
import re

from svo_raytracer_amd import hiplib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["svo_brush_sphere", "svo_brush_box", "svo_pool_download_range", "svo_brush_info", "svo_group_brush_sphere",
         "svo_group_brush_box"]
NATIVES = ["nBrushSphere", "nBrushBox", "nPoolDownloadRange", "nBrushInfo", "nGroupBrushSphere", "nGroupBrushBox"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_brush_names_in_header_binding_and_library():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "svo_hip.h"), flags=re.S)
    L = hiplib.lib()
    for n in NAMES:
        assert re.search(r"\bint %s\s*\(" % n, hdr), n
        assert n in hiplib.EXPORTS, n
        assert hasattr(L, n), n
    for lp in (hiplib.CXXLOOP_LIB_PATH, hiplib.VARIANTS_LIB_PATH):      # the comparing builds carry the brush too
        if os.path.exists(lp):
            assert all(hasattr(hiplib.lib(lp), n) for n in NAMES), lp
    for m in ("brush_sphere", "brush_box", "brush_info", "pool_download_range"):
        assert hasattr(hiplib.HipContext, m), m
    for m in ("brush_sphere", "brush_box"):
        assert hasattr(hiplib.HipGroup, m), m


def test_brush_natives_in_jni_header_library_and_twin():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "svo_hip_jni.h"), flags=re.S)
    java = _read("integration", "java", "src", "engine", "HipRenderer.java")
    L = hiplib.lib()
    for n in NATIVES:
        assert re.search(r"\bj\w+ Java_src_engine_HipRenderer_%s\(" % n, hdr), n
        assert hasattr(L, "Java_src_engine_HipRenderer_" + n), n
        assert re.search(r"private static native \w+ %s\(" % n, java), n
        assert len(re.findall(r"\b%s\(" % n, java)) >= 2, n        # declared and called
    for m in ("brushSphere", "brushBox", "placeSDF"):
        assert len(re.findall(r"\b%s\(" % m, java)) >= 2, m        # on HipRenderer and on HipRenderer.Group
    host = _read("svo-raytracer_amd", "host", "svo_host.hpp")
    assert "svo_brush_sphere" in host and "svo_brush_box" in host


def test_null_context_is_refused_without_a_gpu():
    L = hiplib.lib()
    org = (ctypes.c_int * 3)(1, 2, 3)
    cb = (ctypes.c_int32 * 4)()
    buf = (ctypes.c_uint8 * 16)()
    assert L.svo_brush_sphere(None, org, 4, 1, 64, 6, cb) == -1            # SVO_E_INVALID
    assert L.svo_brush_box(None, org, 4, 4, 4, 1, 64, 6, cb) == -1
    assert L.svo_pool_download_range(None, buf, 0, 16) == -1
    assert L.svo_brush_info(None, None, None, None, None, None, None) == -1
    assert L.svo_group_brush_sphere(None, org, 4, 1, 64, 6, cb) == -1
    assert L.svo_group_brush_box(None, org, 4, 4, 4, 1, 64, 6, cb) == -1
    P = "Java_src_engine_HipRenderer_"
    vp, jint, jlong = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    f = getattr(L, P + "nBrushSphere")
    f.restype, f.argtypes = jint, [vp, vp, jlong] + [jint] * 7 + [jlong]
    assert f(None, None, 0, 1, 2, 3, 4, 1, 64, 6, 0) == -1
    f = getattr(L, P + "nBrushInfo")
    f.restype, f.argtypes = jlong, [vp, vp, jlong, jlong, jlong]
    assert f(None, None, 0, 0, 0) == -1
