"""The general tracer's ray-query hierarchy in the public interface, without a GPU: the header's
flag and feature macro, the Python binding's copy of the flag, and the debug export's declaration."""
import os
import re

from eray_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defines(path):
    with open(path) as f:
        return dict(re.findall(r"^#define\s+(ERAY_\w+)\s+(\w+)", f.read(), re.M))


def test_header_flag_and_feature_macro():
    d = _defines(os.path.join(ROOT, "include", "eray_hip.h"))
    assert d.get("ERAY_HAS_TRACE_RAY_ACCEL") == "1"
    assert d["ERAY_RENDER_NO_RAY_ACCEL"] == "64u"
    assert capi.RENDER_NO_RAY_ACCEL == int(d["ERAY_RENDER_NO_RAY_ACCEL"].rstrip("u"))
    assert d["ERAY_ABI_VERSION"] == "6"  # a new flag and a new debug export: the ABI stays


def test_render_flags_are_distinct_bits():
    d = _defines(os.path.join(ROOT, "include", "eray_hip.h"))
    flags = {k: int(v.rstrip("u")) for k, v in d.items() if k.startswith("ERAY_RENDER_") and k != "ERAY_RENDER_DEFAULT"}
    assert len(set(flags.values())) == len(flags)
    assert all(v and not (v & (v - 1)) for v in flags.values()), flags
    assert sum(flags.values()) == 127  # bit 128 is the first unknown one


def test_debug_export_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "eray_hip_debug.h")) as f:
        assert re.search(r"int\s+eray_debug_trace_ray_accel\(eray_ctx\*\s*ctx,\s*uint32_t\*\s*objects\);", f.read())
    assert hasattr(capi.Context, "trace_ray_accel_objects")


def test_library_exports_the_debug_entry_point():
    """Loads the library (no device call): a null context is refused, not dereferenced."""
    assert capi.lib().eray_debug_trace_ray_accel(None, None) == capi.E_INVALID_ARGUMENT
