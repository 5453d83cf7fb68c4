"""eray_rays_reach_light's boundary on the host (no GPU): capi.ReachParams has the size and the
field offsets include/eray_hip.h states for eray_reach_params, the header announces the entry with
ERAY_HAS_REACH_LIGHT and the secondary rays' use of the hierarchy with ERAY_HAS_RAY_ACCEL_SECONDARY
(ERAY_ABI_VERSION stays 6), the symbol is exported, and a null context is an error.  (The header
parser is tests/test_rays_host.py's, copied.)"""
import ctypes as C
import os
import re

from eray_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "eray_hip.h")).read()


def header_struct(name):
    """(size from the struct's 'NN B' comment, {field: offset} from its 'offset N' comments)."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S)
    assert m, name
    body = m.group(1)
    size = int(re.search(r"(\d+) B \*/", body).group(1))
    offsets = {}
    for decl, first, second in re.findall(r"([^;/]*);\s*/\* offset (\d+)(?:, (\d+))?", body):
        names = [re.sub(r"\[.*", "", n.strip().split()[-1].lstrip("*")) for n in decl.split(",")]
        for n, off in zip(names, [first, second]):
            offsets[n] = int(off)
    return size, offsets


def test_reach_params_matches_the_header():
    hsize, offsets = header_struct("eray_reach_params")
    assert hsize == 40 == C.sizeof(capi.ReachParams)
    assert offsets == {"rays": 0, "targets": 8, "count": 16, "flags": 24, "reserved": 28, "out": 32}
    assert set(offsets) == {f[0] for f in capi.ReachParams._fields_}
    for field, off in offsets.items():
        assert getattr(capi.ReachParams, field).offset == off, field


def test_header_announces_the_additions():
    assert re.search(r"^#define ERAY_HAS_RAY_ACCEL_SECONDARY 1\b", HEADER, re.M)
    assert re.search(r"^#define ERAY_HAS_REACH_LIGHT 1\b", HEADER, re.M)
    assert re.search(r"^#define ERAY_ABI_VERSION 6\b", HEADER, re.M)
    assert re.search(r"^int eray_rays_reach_light\(eray_ctx\* ctx, const eray_reach_params\* params\);", HEADER, re.M)


def test_symbol_is_exported_and_bound():
    assert "eray_rays_reach_light" in capi.SIGNATURES
    restype, argtypes = capi.SIGNATURES["eray_rays_reach_light"]
    assert restype is C.c_int and argtypes[1] is C.POINTER(capi.ReachParams)
    assert hasattr(capi.lib(), "eray_rays_reach_light")
    assert hasattr(capi.Context, "rays_reach_light") and hasattr(capi.Context, "rays_reach_light_device")


def test_null_context_is_an_error_not_a_crash():
    p = capi.ReachParams(None, None, 0, 0, 0, None)
    assert capi.lib().eray_rays_reach_light(None, C.byref(p)) == capi.E_INVALID_ARGUMENT
    assert capi.lib().eray_rays_reach_light(None, None) == capi.E_INVALID_ARGUMENT
