"""The channeliser's integer-capture entry points, host side (no GPU): fmd_chan_process_u8_dev / _s8_dev / _s16_dev are exported and
refuse missing arguments with FMD_ERR_ARG before they touch a handle or a device."""
import ctypes as C

import pytest

import fmradio_loader

FORMATS = ("u8", "s8", "s16")
FMD_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    p = fmradio_loader.load()
    p.build_library()
    return p.load_library()


@pytest.mark.parametrize("fmt", FORMATS)
def test_entry_point_is_exported_and_declared(lib, fmt):
    import fmradio_loader as fl
    name = f"fmd_chan_process_{fmt}_dev"
    assert hasattr(lib, name)
    assert name in fl.load().declared_symbols(debug=False)
    assert lib.fmd_api_version() == 3


@pytest.mark.parametrize("fmt", FORMATS)
def test_missing_arguments_are_refused(lib, fmt):
    fn = getattr(lib, f"fmd_chan_process_{fmt}_dev")
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    # stand-ins for device buffers and a handle: the argument check comes first, so none of them is dereferenced (zeroed host memory,
    # should that ever change)
    handle, wide, out = (C.create_string_buffer(4096) for _ in range(3))
    got = C.c_size_t(12345)
    h, w, o = C.addressof(handle), C.addressof(wide), C.addressof(out)
    assert fn(None, w, 625, o, 16, C.byref(got), None) == FMD_ERR_ARG
    assert fn(h, None, 625, o, 16, C.byref(got), None) == FMD_ERR_ARG
    assert fn(h, w, 625, None, 16, C.byref(got), None) == FMD_ERR_ARG
    assert fn(h, w, 625, o, 16, None, None) == FMD_ERR_ARG
    assert got.value == 12345                                # nothing reported
    assert handle.raw == b"\0" * 4096 and out.raw == b"\0" * 4096
