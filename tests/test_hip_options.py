"""The option table of libdcvc_hip (options.h): every name dcvc_set_option
takes, with its default, reads back through dcvc_get_option.

The table below is literal on purpose: an option that disappears, changes its
name or changes its default fails here.  Setting an option touches no GPU (the
registry holds plain ints), so this runs on hosts without one.
"""
import pytest

from dcvc_amd._native import NativeError

DEFAULTS = {
    "gemm1x1": 1,
    "gemm1x1_f32": 1,
    "gemm3x3_f32": 1,
    "gemm1x1_f32_cfg": 0,
    "gemm1x1_f32_upfront": 1,
    "gemm1x1_f32_direct": 1,
    "conv3x3": 1,
    "dcb_persistent": 1,
    "conv3x3_s2": 1,
    "conv7_wide_cin": 1,
    "conv7_small_cin": 1,
    "dcb_stream": 1,
    "conv3x3_persistent": 1,
    "conv3x3_resident": 1,
    "conv_th": 0,
    "conv_bn": 0,
    "gemm1x1_bm": 0,
    "conv3x3_occupancy": 1,
    "conv3x3_epilogue": 0,
    "sconv_res_waves": 0,
    "sgemm_pd": 0,
    "sgemm_gate": 1,
    "sgemm": 0,
    "sconv_resident": 1,
    "sconv_waves": 8,
    "sconv_occupancy": 0,
    "xconv": 1,
    "wconv": 0,
    "dconv": 1,
    "dconv_1x1": 1,
    "sffn128": 1,
    "nconv": 1,
    "tconv": 1,
    "dconv_xcd": 1,
    "dconv_gate": 1,
    "dconv_s2blocks": 2,
    "dconv_bn128": 1,
    "conv3x3_rows4": 1,
    "sconv_dbg": 0,
    "sconv_rw": 0,
    "xconv_dbg": 0,
    "xconv_rw1": 1,
    "wconv_dbg": 0,
}


def K():
    from dcvc_amd import hip
    return hip


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_option_default_and_round_trip(name):
    h = K()
    default = DEFAULTS[name]
    assert h.get_option(name) == default
    try:
        for v in (default + 3, -1, 0, 128, 77):   # 128: a value "gemm1x1_bm" acts on, 77: one it ignores
            h.set_option(name, v)
            assert h.get_option(name) == v
    finally:
        h.set_option(name, default)
    assert h.get_option(name) == default


def test_setting_one_option_leaves_the_others():
    h = K()
    try:
        h.set_option("dconv", 5)
        got = {n: h.get_option(n) for n in DEFAULTS}
    finally:
        h.set_option("dconv", DEFAULTS["dconv"])
    assert got == {**DEFAULTS, "dconv": 5}


@pytest.mark.parametrize("name", ["", "no_such_option", "dconv ", "DCONV", "dconv_"])
def test_unknown_option_raises(name):
    h = K()
    with pytest.raises(NativeError):
        h.set_option(name, 1)
    with pytest.raises(NativeError):
        h.get_option(name)
    assert {n: h.get_option(n) for n in DEFAULTS} == DEFAULTS
