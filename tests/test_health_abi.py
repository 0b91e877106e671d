"""CPU-side checks of the device health words: header, ctypes table and the config validation agree."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "mobody_hip.h")).read()


def _define(name):
    m = re.search(r"^#define\s+%s\s+(\S+)" % name, _header(), flags=re.M)
    assert m, f"{name} is not defined in the header"
    return m.group(1)


def test_health_prototypes_and_constants_match_the_header():
    from mobody_amd import _lib
    import ctypes as C
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+mobody_health_bind\s*\(\s*int32_t\s*\*\s*words_dev\s*\)\s*;", hdr)
    assert re.search(r"int\s+mobody_health_clear\s*\(\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    assert _lib.PROTOTYPES["mobody_health_bind"] == (C.c_int, [C.c_void_p])
    assert _lib.PROTOTYPES["mobody_health_clear"] == (C.c_int, [C.c_void_p])
    assert _lib.HEALTH_WORDS == int(_define("MOBODY_HEALTH_WORDS")) >= 4
    assert _lib.HEALTH_F16_RANGE == int(_define("MOBODY_HEALTH_F16_RANGE"))
    assert _lib.HEALTH_NONFINITE == int(_define("MOBODY_HEALTH_NONFINITE"))
    assert _lib.HEALTH_F16_RANGE & _lib.HEALTH_NONFINITE == 0
    assert int(_define("MOBODY_ABI_VERSION")) == 7            # the health entry points themselves are as in version 6


def test_f16_weight_limit_is_the_headers_bound():
    from mobody_amd import ops
    assert ops.F16_W_LIMIT == 65504 / 2 ** 8
    assert float(_define("MOBODY_F16_W_LIMIT").rstrip("f")) == ops.F16_W_LIMIT
    src = open(os.path.join(ROOT, "mobody-model-based-off-dynamics-offline-reinforcement-learning_amd", "csrc", "tile_bf.h")).read()
    assert re.search(r"constexpr int F16_WSHIFT = 8;", src)   # the shift both bounds are derived from


def test_f16_guard_validation():
    from mobody_amd import ops
    for ok in ("raise", "fallback", "off"):
        assert ops.check_f16_guard(ok) == ok
    for bad in ("", "warn", "Raise", None, 1):
        with pytest.raises(ValueError):
            ops.check_f16_guard(bad)
    with pytest.raises(ValueError):
        ops.check_f16_guard("fallback", distributed=True)
    assert ops.check_f16_guard("raise", distributed=True) == "raise"
    assert ops.check_f16_guard("off", distributed=True) == "off"
