"""CPU-side checks of compaction's boundary (svo_pool_compact / svo_compact_info / svo_group_pool_compact): declared in the
header, listed by the binding, exported by every build of the library with their JNI natives and the Java twin's methods, and
a null context is refused, not dereferenced.  The level bound is stated once, from the walker's stack."""
import ctypes
import os
import re

from svo_raytracer_amd import hiplib
import compact_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["svo_pool_compact", "svo_compact_info", "svo_group_pool_compact"]
NATIVES = ["nPoolCompact", "nCompactInfo", "nGroupPoolCompact"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_compact_names_in_header_binding_and_library():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "svo_hip.h"), flags=re.S)
    L = hiplib.lib()
    for n in NAMES:
        assert re.search(r"\bint %s\s*\(" % n, hdr), n
        assert n in hiplib.EXPORTS, n
        assert hasattr(L, n), n
    for lp in (hiplib.CXXLOOP_LIB_PATH, hiplib.VARIANTS_LIB_PATH):
        if os.path.exists(lp):
            assert all(hasattr(hiplib.lib(lp), n) for n in NAMES), lp
    for m in ("pool_compact", "compact_info"):
        assert hasattr(hiplib.HipContext, m), m
    assert hasattr(hiplib.HipGroup, "pool_compact")


def test_compact_natives_in_jni_header_library_and_twin():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "svo_hip_jni.h"), flags=re.S)
    java = _read("integration", "java", "src", "engine", "HipRenderer.java")
    L = hiplib.lib()
    for n in NATIVES:
        assert re.search(r"\bj\w+ Java_src_engine_HipRenderer_%s\(" % n, hdr), n
        assert hasattr(L, "Java_src_engine_HipRenderer_" + n), n
        assert re.search(r"private static native \w+ %s\(" % n, java), n
        assert len(re.findall(r"\b%s\(" % n, java)) >= 2, n        # declared and called
    assert len(re.findall(r"\bcompactPool\(", java)) >= 2          # on HipRenderer and on HipRenderer.Group
    assert "svo_pool_compact" not in _read("svo-raytracer_amd", "host", "svo_host.hpp")   # svo::host::Octree is the reference's class


def test_null_context_is_refused_without_a_gpu():
    L = hiplib.lib()
    assert L.svo_pool_compact(None, None, None) == -1              # SVO_E_INVALID
    assert L.svo_compact_info(None, None, None, None, None) == -1
    assert L.svo_group_pool_compact(None, None, None) == -1
    P = "Java_src_engine_HipRenderer_"
    vp, jint, jlong = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    sizes = (ctypes.c_int64 * 2)(5, 5)
    for name in ("nPoolCompact", "nGroupPoolCompact"):
        f = getattr(L, P + name)
        f.restype, f.argtypes = jint, [vp, vp, jlong, jlong]
        assert f(None, None, 0, ctypes.addressof(sizes)) == -1 and list(sizes) == [0, 0]
    f = getattr(L, P + "nCompactInfo")
    f.restype, f.argtypes = jlong, [vp, vp, jlong, jlong, jlong]
    assert f(None, None, 0, 0, 0) == -1


def test_the_level_bound_is_the_walkers_stack():
    dev = _read("svo-raytracer_amd", "csrc", "svo_device.h")
    src = _read("svo-raytracer_amd", "csrc", "svo_compact.hip.h")
    stack = int(re.search(r"constexpr int kStackLevels = (\d+);", dev).group(1))
    assert re.search(r"constexpr int kMaxLevels = kStackLevels \+ 1;", src)
    assert compact_ref.MAX_LEVELS == stack + 1
