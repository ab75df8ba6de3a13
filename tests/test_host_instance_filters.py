"""CPU tests of filter functions on instanced meshes (device config inst_filters=1) on a host-only device: the key, what the top scene's
commit takes and records, what stays refused.  The traversal side is tests/test_gpu_instance_filters.py."""
import ctypes as C

import numpy as np
import pytest

import inst_filter_helpers as fh
import instance_helpers as ih

ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)
KEYED = fh.HOST_CFG + ",inst_filters=1"


class Errors:
    """the messages the device reports through rtcSetDeviceErrorFunction"""

    def __init__(self, dev):
        self.log = []
        self.fn = ERRFN(lambda user, code, msg: self.log.append((code, (msg or b"").decode())))
        dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(self.fn, C.c_void_p), None)
        self.dev = dev

    def expect(self, code, text):
        assert self.dev.error() == code, self.log
        assert self.log and self.log[-1][0] == code and text in self.log[-1][1], self.log
        self.log.clear()


def _top_over(rtc, dev, inner, n=2):
    top = rtc.Scene(dev)
    for i in range(n):
        top.add_instance(inner, ih.affine((2.0 * i, 0, 0)))
    return top


@pytest.mark.parametrize("quads", [False, True])
def test_a_filter_inside_an_instanced_mesh_scene_commits_with_the_key(rtc, quads):
    dev = rtc.Device(KEYED)
    fn = rtc.FILTER_FUNC(lambda args: None)
    inner = fh.stack_scene(rtc, dev, quads)
    inner.set_filters(1, intersect=fn)
    inner.commit()
    top = _top_over(rtc, dev, inner)
    top.commit()
    assert top.stats()["accelKind"] in ((16, 17) if quads else (14, 15))
    assert top.filter_flags() == rtc.RTCAMD_SCENE_FILTER_INSTANCED_INTERSECT
    top.release()
    inner.release()
    dev.release()


@pytest.mark.parametrize("cfg", [fh.HOST_CFG, fh.HOST_CFG + ",inst_filters=0"])
def test_without_the_key_the_commit_is_refused_with_the_old_text(rtc, cfg):
    dev = rtc.Device(cfg)
    err = Errors(dev)
    fn = rtc.FILTER_FUNC(lambda args: None)
    for which in ("intersect", "occluded"):
        inner = fh.stack_scene(rtc, dev)
        inner.set_filters(2, **{which: fn})
        inner.commit()
        top = _top_over(rtc, dev, inner)
        top.lib.rtcCommitScene(top.handle)
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "geometry filter functions inside an instanced scene are not supported")
        top.release()
        inner.release()
    dev.release()


@pytest.mark.parametrize("val", ["2", "", "yes", "-1"])
def test_any_other_value_of_the_key_is_an_invalid_argument(rtc, val):
    with pytest.raises(rtc.RTCError) as e:
        rtc.Device("gpu=none,inst_filters=" + val)
    assert e.value.code == rtc.RTC_ERROR_INVALID_ARGUMENT  # (the message names the key and "(0 or 1)"; no device exists to report it to)


def test_a_filter_on_subdivision_geometry_below_an_instance_stays_refused(rtc):
    dev = rtc.Device("gpu=none,inst_accel=default,subdiv_accel=default,quad_accel=default,inst_filters=1")
    err = Errors(dev)
    fn = rtc.FILTER_FUNC(lambda args: None)
    inner = rtc.Scene(dev)
    inner.add_subdiv(fh.SQUARE, np.array([4], np.uint32), np.arange(4, dtype=np.uint32))
    inner.set_levels(2, 1)
    inner.set_filters(0, intersect=fn)
    inner.commit()
    top = _top_over(rtc, dev, inner, 1)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "subdivision geometry with a filter function inside an instanced scene is not supported")
    top.release()
    inner.release()
    dev.release()


def test_the_recorded_flags_follow_the_filters_of_enabled_geometries(rtc):
    dev = rtc.Device(KEYED)
    fn = rtc.FILTER_FUNC(lambda args: None)
    I, O = rtc.RTCAMD_SCENE_FILTER_INSTANCED_INTERSECT, rtc.RTCAMD_SCENE_FILTER_INSTANCED_OCCLUDED
    inner = fh.stack_scene(rtc, dev)
    inner.commit()
    top = _top_over(rtc, dev, inner)
    top.commit()
    assert top.filter_flags() == 0
    for intersect, occluded, want in ((fn, None, I), (None, fn, O), (fn, fn, I | O), (None, None, 0)):
        inner.set_filters(3, intersect=intersect, occluded=occluded)
        inner.commit()
        # the instanced scene's own flags are the ones it always had; the top scene's are what ITS commit sees
        assert inner.filter_flags() == (rtc.RTCAMD_SCENE_FILTER_MESH_INTERSECT if intersect else 0) | (rtc.RTCAMD_SCENE_FILTER_MESH_OCCLUDED if occluded else 0)
        top.commit()
        assert top.filter_flags() == want
    # a disabled geometry does not count, in the instanced scene ...
    inner.set_filters(3, intersect=fn, occluded=fn)
    inner.set_enabled(3, False)
    inner.commit()
    top.commit()
    assert top.filter_flags() == 0
    inner.set_enabled(3, True)
    inner.commit()
    top.commit()
    assert top.filter_flags() == I | O
    # ... and neither does the scene of a disabled instance
    other = fh.stack_scene(rtc, dev)
    other.commit()
    top2 = rtc.Scene(dev)
    a = top2.add_instance(inner, ih.affine((0, 0, 0)))
    top2.add_instance(other, ih.affine((2.0, 0, 0)))
    top2.commit()
    assert top2.filter_flags() == I | O
    top2.set_enabled(a, False)
    top2.commit()
    assert top2.filter_flags() == 0
    for s in (top2, top, other, inner):
        s.release()
    dev.release()


def test_the_equivalence_cases_keep_their_ties_below_one_percent(rtc, po):
    """the CPU part of the GPU equivalence test: the pinned seed, by the oracle alone"""
    for form in fh.EQ_KINDS:
        if form == "meshmb_linear":
            continue  # the rays and meshes of "meshmb"
        for mode in (0, 1):
            fh.equivalence_case(rtc, po, form, mode)
