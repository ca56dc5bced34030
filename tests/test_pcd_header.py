"""The host half of the PointCloud.pcd export (include/dmsa_wire_formats.h): the header text of a PointCloud<PointNormal> and the exports
of the device half.  No GPU needed."""
import ctypes as C

import pytest

from dmsa_lidar_slam_amd import _capi as capi


def expected_header(n: int) -> bytes:
    return (
        "# .PCD v0.7 - Point Cloud Data file format\n"
        "VERSION 0.7\n"
        "FIELDS x y z normal_x normal_y normal_z curvature\n"
        "SIZE 4 4 4 4 4 4 4\n"
        "TYPE F F F F F F F\n"
        "COUNT 1 1 1 1 1 1 1\n"
        f"WIDTH {n}\n"
        "HEIGHT 1\n"
        "VIEWPOINT 0 0 0 1 0 0 0\n"
        f"POINTS {n}\n"
        "DATA ascii\n"
    ).encode()


@pytest.mark.parametrize("n", [1, 17_887, 2_500_000, 2**31 + 5])
def test_header_bytes(n):
    lib = capi.load_library()
    buf = C.create_string_buffer(512)
    rc = lib.dmsa_pcd_header_pointnormal(n, buf, 512)
    want = expected_header(n)
    assert rc == len(want)
    assert buf.raw[:rc] == want and buf.raw[rc] == 0


def test_header_capacity():
    lib = capi.load_library()
    need = len(expected_header(17_887))
    buf = C.create_string_buffer(512)
    assert lib.dmsa_pcd_header_pointnormal(17_887, buf, need) < 0  # no room for the terminating 0
    assert lib.dmsa_pcd_header_pointnormal(17_887, buf, 16) < 0
    assert lib.dmsa_pcd_header_pointnormal(17_887, buf, 0) < 0
    assert lib.dmsa_pcd_header_pointnormal(17_887, None, 512) < 0
    assert lib.dmsa_pcd_header_pointnormal(-1, buf, 512) < 0
    assert lib.dmsa_pcd_header_pointnormal(17_887, buf, need + 1) == need


def test_python_mirror_header():
    from dmsa_lidar_slam_amd import wire_formats

    assert wire_formats.pcdHeaderPointNormal(17_887).encode() == expected_header(17_887)


def test_exports():
    lib = capi.load_library()
    for name in ("dmsa_get_global_normals", "dmsa_format_pcd_rows", "dmsa_save_pcd_ascii", "dmsa_save_pcd_ascii_ex", "dmsa_pcd_header_pointnormal"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED_SYMBOLS


def test_null_context_is_refused():
    """The device entry points check their arguments on the host before anything else."""
    lib = capi.load_library()
    used = C.c_int64(7)
    fnull = capi.ptr(None, C.c_float)
    assert lib.dmsa_format_pcd_rows(None, fnull, fnull, fnull, 0, 1, None, 0, C.byref(used)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_save_pcd_ascii(None, b"unused.pcd", fnull, fnull, fnull, 1, C.byref(used)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_get_global_normals(None, fnull, 0) == capi.DMSA_ERR_INVALID
