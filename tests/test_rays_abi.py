"""CPU-side checks of the ray queries' boundary (svo_cast_rays / svo_cast_rays_device / svo_cast_info): declared in the
header with the arity the binding and the JNI shim use, exported by every built library, with their JNI natives and the
Java twin's declarations, and a null context is refused, not dereferenced."""
import ctypes
import os
import re

from svo_raytracer_amd import hiplib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"svo_cast_rays": 4, "svo_cast_rays_device": 4, "svo_cast_info": 6}
NATIVES = {"nCastRays": 4, "nCastInfo": 3}      # parameters behind env, cls


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_ray_names_in_header_binding_and_every_library():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "svo_hip.h"), flags=re.S)
    for n, arity in ARITY.items():
        m = re.search(r"\bint %s\s*\(([^)]*)\);" % n, hdr)
        assert m, n
        assert len(m.group(1).split(",")) == arity, (n, m.group(1))
        assert n in hiplib.EXPORTS, n
        assert len(getattr(hiplib.lib(), n).argtypes) == arity, n
    built = [p for p in (hiplib.LIB_PATH, hiplib.CXXLOOP_LIB_PATH, hiplib.VARIANTS_LIB_PATH) if os.path.exists(p)]
    assert hiplib.LIB_PATH in built and len(built) == 3, built      # build() makes all three
    for lp in built:
        assert all(hasattr(hiplib.lib(lp), n) for n in ARITY), lp
    for m in ("cast_rays", "cast_rays_device", "cast_info"):
        assert callable(getattr(hiplib.HipContext, m)), m
    assert hiplib.HIT_DTYPE.itemsize == 16


def test_ray_natives_in_jni_header_shim_and_twin():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "svo_hip_jni.h"), flags=re.S)
    shim = _read("svo-raytracer_amd", "csrc", "svo_jni.cpp")
    java = _read("integration", "java", "src", "engine", "HipRenderer.java")
    L = hiplib.lib()
    for n, arity in NATIVES.items():
        m = re.search(r"\bj\w+ Java_src_engine_HipRenderer_%s\(([^)]*)\);" % n, hdr)
        assert m and len(m.group(1).split(",")) == arity + 2, n
        assert re.search(r"\bj\w+ Java_src_engine_HipRenderer_%s\(" % n, shim), n
        assert hasattr(L, "Java_src_engine_HipRenderer_" + n), n
        m = re.search(r"private static native \w+ %s\(([^)]*)\);" % n, java)
        assert m and len(m.group(1).split(",")) == arity, n
        assert len(re.findall(r"\b%s\(" % n, java)) >= 2, n        # declared and called
    assert re.search(r"public void castRays\(\s*(java\.nio\.)?FloatBuffer \w+,\s*ByteBuffer \w+\)", java)
    assert re.search(r"public long\[\] castInfo\(\)", java)


def test_null_context_is_refused_without_a_gpu():
    L = hiplib.lib()
    rays = (ctypes.c_float * 6)(1.5, 1.9, 1.5, 0.0, -1.0, 0.0)
    hit = (ctypes.c_uint8 * 16)()
    assert L.svo_cast_rays(None, rays, 1, hit) == -1                # SVO_E_INVALID
    assert L.svo_cast_rays_device(None, rays, 1, hit) == -1
    assert L.svo_cast_info(None, None, None, None, None, None) == -1
    P = "Java_src_engine_HipRenderer_"
    vp, jint, jlong = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    f = getattr(L, P + "nCastRays")
    f.restype, f.argtypes = jint, [vp, vp, jlong, jlong, jint, jlong]
    assert f(None, None, 0, 0, 1, 0) == -1
    assert f(None, None, 0, 0, -1, 0) == -1
    f = getattr(L, P + "nCastInfo")
    f.restype, f.argtypes = jlong, [vp, vp, jlong, jlong, jlong]
    assert f(None, None, 0, 0, 0) == -1
