"""The ray-query boundary on the host (no GPU): the ctypes structures of eray_amd/capi.py have the
sizes and field offsets include/eray_hip.h states for eray_ray, eray_ray_hit and eray_rays_params,
and the header announces the entry with ERAY_HAS_CAST_RAYS (ERAY_ABI_VERSION stays 6)."""
import ctypes as C
import os
import re

import numpy as np

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


def test_structures_match_the_header():
    for name, cls, size in (("eray_ray", capi.Ray, 24), ("eray_ray_hit", capi.RayHit, 48),
                            ("eray_rays_params", capi.RaysParams, 48)):
        hsize, offsets = header_struct(name)
        assert hsize == size == C.sizeof(cls), name
        assert set(offsets) == {f[0] for f in cls._fields_}, name
        for field, off in offsets.items():
            assert getattr(cls, field).offset == off, (name, field)
    assert capi.HIT_DTYPE.itemsize == 48 and capi.RAY_DTYPE.itemsize == 24
    for field, _ in capi.RayHit._fields_:
        assert capi.HIT_DTYPE.fields[field][1] == getattr(capi.RayHit, field).offset, field


def test_header_announces_cast_rays():
    assert re.search(r"^#define ERAY_HAS_CAST_RAYS 1\b", HEADER, re.M)
    assert re.search(r"^#define ERAY_ABI_VERSION 6\b", HEADER, re.M)
    assert re.search(r"^#define ERAY_RAYS_NORMALIZE 1u", HEADER, re.M) and capi.RAYS_NORMALIZE == 1
    assert re.search(r"^#define ERAY_RAYS_BRUTE_FORCE 2u", HEADER, re.M) and capi.RAYS_BRUTE_FORCE == 2
    assert "eray_cast_rays" in capi.SIGNATURES and hasattr(capi.lib(), "eray_cast_rays")


def test_null_context_is_an_error_not_a_crash():
    p = capi.RaysParams(None, 0, -1, 0, 0, None, None)
    assert capi.lib().eray_cast_rays(None, C.byref(p)) == capi.E_INVALID_ARGUMENT
    assert np.dtype(capi.HIT_DTYPE).names == ("object", "face", "position", "normal", "uv", "u", "v")
