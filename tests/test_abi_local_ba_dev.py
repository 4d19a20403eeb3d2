"""CPU: libslamhip.so exports slam_local_ba_batch_dev (and the test aid that downloads a staged window), the header documents its new per-window
code, and the Python wrapper binds it."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_device_input_batch():
    import slam_jl_amd
    from slam_jl_amd import _lib
    lib = _lib.load()
    assert "slam_local_ba_batch_dev" in _lib.SIGNATURES
    same = _lib.SIGNATURES["slam_local_ba_batch"][1]
    dev = _lib.SIGNATURES["slam_local_ba_batch_dev"][1]
    assert len(dev) == len(same) and [i for i, (a, b) in enumerate(zip(same, dev)) if a is not b] == [6, 7, 8, 9, 10, 11]      # the six device arrays
    assert all(dev[i] is ctypes.c_void_p for i in range(6, 12))
    raw = ctypes.CDLL(slam_jl_amd.LIB_PATH)
    assert hasattr(raw, "slam_local_ba_batch_dev") and hasattr(raw, "slam_debug_ba_dev_staged")
    assert lib.slam_local_ba_batch_dev.argtypes == dev


def test_library_exports_the_estimator_step_on_the_map():
    import slam_jl_amd as slam
    from slam_jl_amd import _lib
    _lib.load()
    raw = ctypes.CDLL(slam.LIB_PATH)
    assert hasattr(raw, "slam_kfmap_local_ba") and hasattr(raw, "slam_kfmap_last_windows")
    vp, i32p, f64p = ctypes.c_void_p, _lib.i32p, _lib.f64p
    assert _lib.SIGNATURES["slam_kfmap_local_ba"] == (ctypes.c_int, [vp, vp, vp, i32p, f64p, ctypes.c_int, ctypes.c_int, ctypes.c_double, i32p, f64p])
    src = inspect.getsource(slam.KeyframeMap.local_ba)
    assert "slam_kfmap_local_ba" in src
    p = inspect.signature(slam.KeyframeMap.local_ba).parameters
    assert list(p)[:4] == ["self", "min_cov_score", "cams", "ks"] and p["ks"].default is None
    b = inspect.signature(slam.bundle_adjustment_batch_).parameters
    assert all(p[k].default == b[k].default for k in ("iterations", "repr_eps", "iters_fast"))


def test_header_documents_the_code_and_the_wrapper_binds_the_entry_point():
    import slam_jl_amd as slam
    hdr = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    m = re.search(r"SLAM_BA_DEV_INELIGIBLE\s*=\s*(-?\d+)", hdr)
    assert m and int(m.group(1)) == slam.SLAM_BA_DEV_INELIGIBLE
    assert int(m.group(1)) not in (0, 1, 2, 3) and int(m.group(1)) > 0          # not an error code, and none of the gather's per-stream codes
    assert "slam_local_ba_batch_dev(" in re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    src = inspect.getsource(slam.bundle_adjustment_batch_dev_)
    assert "slam_local_ba_batch_dev" in src
    assert list(inspect.signature(slam.bundle_adjustment_batch_dev_).parameters)[:10] == [
        "cameras", "Pn", "Mn", "On", "theta", "theta_const", "pixels", "poses_ids", "points_ids", "outliers"]
    d = inspect.signature(slam.bundle_adjustment_batch_dev_).parameters
    b = inspect.signature(slam.bundle_adjustment_batch_).parameters
    assert all(d[k].default == b[k].default for k in ("iterations", "repr_eps", "iters_fast"))
