"""CPU-side checks of include/dmsa_dense_intensity.h: the symbol list, the struct, the two header texts (I7), the sensors' intensity fields
(I5), the null-object refusals, and the model's field conversion (tests/dense_intensity_model.py, the yardstick of the GPU tests) on the
values whose rounding the rules name."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import dense_cloud as dcl

import dense_intensity_model as im
import wire_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_intensity.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header))
    assert declared == set(capi.DENSE_INTENSITY_SYMBOLS) and len(capi.DENSE_INTENSITY_SYMBOLS) == len(declared) == 7
    others = (set(capi.EXPORTED_SYMBOLS) | set(capi.DENSE_CLOUD_SYMBOLS) | set(capi.DENSE_NORMALS_SYMBOLS) | set(capi.DENSE_OUTLIERS_SYMBOLS) |
              set(capi.DENSE_CARVE_SYMBOLS))
    assert not declared & others
    for name in declared:
        assert hasattr(lib, name), name
    for rule in ("I1", "I2", "I3", "I4", "I5", "I6", "I7"):
        assert re.search(rf"\b{rule}\b", header)
    assert "DECIDED HERE" in header and "RECALLED" in header


def test_struct_sizes_and_offsets():
    assert C.sizeof(capi.PointCloud2Field) == 8 and capi.PointCloud2Field.index.offset == 0 and capi.PointCloud2Field.datatype.offset == 4
    assert C.sizeof(capi.DenseConfig) == 96  # the switch is a call, not a field
    assert C.sizeof(capi.DenseStats) == 64
    assert capi.FIELD_DATATYPES == {"int8": 1, "uint8": 2, "int16": 3, "uint16": 4, "int32": 5, "uint32": 6, "float32": 7, "float64": 8}


@pytest.mark.parametrize("call,fields", [("dmsa_pcd_header_xyzi_binary", "x y z intensity"),
                                         ("dmsa_pcd_header_xyzi_normals_binary", "x y z intensity normal_x normal_y normal_z curvature")])
def test_headers_are_their_stated_text(lib, call, fields):
    k = len(fields.split())
    py = dcl.pcdHeaderXyziBinary if k == 4 else dcl.pcdHeaderXyziNormalsBinary
    model = im.header_xyzi if k == 4 else im.header_xyzi_normals
    lengths = set()
    for n in (0, 1, 10**12 - 1):
        want = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS " + fields + "\nSIZE" + " 4" * k + "\nTYPE" + " F" * k + "\nCOUNT" + " 1" * k +
                "\nWIDTH %012d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012d\nDATA binary\n" % (n, n))
        assert py(n) == want == model(n)
        lengths.add(len(want))
    assert len(lengths) == 1  # the counts are patched in place
    size = lengths.pop()
    fn, buf = getattr(lib, call), C.create_string_buffer(512)
    assert fn(10**12, buf, 512) == capi.DMSA_ERR_INVALID and fn(-1, buf, 512) == capi.DMSA_ERR_INVALID
    assert fn(5, buf, size) == capi.DMSA_ERR_INVALID and fn(5, buf, size + 1) == size  # room for the terminating zero, as the x y z twins
    assert fn(5, None, 512) == capi.DMSA_ERR_INVALID and fn(5, buf, 0) == capi.DMSA_ERR_INVALID
    # the lines that are not about fields are those of the twin
    twin = dcl.pcdHeaderXyzBinary(77) if k == 4 else dcl.pcdHeaderNormalsBinary(77)
    assert [a for a in py(77).splitlines() if a.split()[0] not in ("FIELDS", "SIZE", "TYPE", "COUNT")] == \
           [a for a in twin.splitlines() if a.split()[0] not in ("FIELDS", "SIZE", "TYPE", "COUNT")]


def test_sensor_intensity_field_for_all_eight_sensors(lib):
    assert len(capi.SENSORS) == 8
    for name, sensor in capi.SENSORS.items():
        f = capi.PointCloud2Field(99, 99)
        rc = lib.dmsa_sensor_intensity_field(sensor, C.byref(f))
        if name in ("sick", "unknown"):
            assert rc == capi.DMSA_ERR_INVALID and (f.index, f.datatype) == (99, 99)
            with pytest.raises(dcl.DmsaError):
                dcl.sensor_intensity_field(name)
            continue
        assert rc == capi.DMSA_OK and (f.index, f.datatype) == (3, 7) == dcl.sensor_intensity_field(name)
        # ... which is the fourth field of the layout tests/wire_util.py states, a float32
        fields = [f for f in wire_util.LAYOUTS[name] if f[0] not in wire_util._PADS]
        assert fields[3][0] in ("intensity", "reflectivity") and fields[3][1] == "<f4"
    assert lib.dmsa_sensor_intensity_field(-1, C.byref(f)) == capi.DMSA_ERR_INVALID and lib.dmsa_sensor_intensity_field(8, C.byref(f)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_sensor_intensity_field(0, None) == capi.DMSA_ERR_INVALID
    with pytest.raises(ValueError):
        dcl.sensor_intensity_field("lidar9000")


def test_null_objects_are_refused(lib):
    f, kept = capi.PointCloud2Field(3, 7), C.c_int64(5)
    assert lib.dmsa_dense_cloud_with_intensity(None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_has_intensity(None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_decode_pointcloud2_field(None, None, C.byref(f), None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_add_pointcloud2_field(None, None, 0, C.byref(f), None, 0, C.byref(kept), None) == capi.DMSA_ERR_INVALID and kept.value == 0


def test_the_models_conversion_rounds_to_nearest_even():
    """The yardstick of the GPU test, on the halfway cases I4 names: numpy's astype is the C conversion."""
    def conv(values, datatype):
        raw = np.array(values, im.DATATYPES[datatype])
        return im.field_as_float32(np.frombuffer(raw.tobytes(), np.uint8), raw.shape[0], raw.dtype.itemsize, 0, datatype)

    assert list(conv([2**24 + 1, -(2**24 + 1), 2**24 + 3, 2**31 - 1], 5)) == [2.0**24, -(2.0**24), 2.0**24 + 4, 2.0**31]
    assert list(conv([2**24 + 1, 2**24 + 3, 2**32 - 1], 6)) == [2.0**24, 2.0**24 + 4, 2.0**32]
    got = conv([1e39, -1e39, 2.0**-150, 1.5 * 2.0**-149, 1.0 + 2.0**-24, 1.0 + 3 * 2.0**-24], 8)
    assert list(got) == [np.inf, -np.inf, 0.0, 2.0**-148, 1.0, 1.0 + 2.0**-22]
    nan = conv(np.array([0x7FC12345, 0x00000001, 0x80000000], np.uint32).view(f32), 7)
    assert list(nan.view(np.uint32)) == [0x7FC12345, 1, 0x80000000]
