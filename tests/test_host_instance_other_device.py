"""An instance names a scene of its own device only (rtcSetGeometryInstancedScene refuses any other, as rtcAttachGeometry refuses a
geometry of another device).  One device has one mb_bounds, so the motion-blur trees below one top scene are all of one node type: what
the instance accels of inst_mb_bounds=linear rely on."""
import ctypes as C

import numpy as np

from helpers import random_soup

BASE = "gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default"


def test_an_instance_cannot_name_a_scene_of_another_device(rtc):
    d0, d1 = rtc.Device(BASE + ",mb_bounds=linear,inst_mb_bounds=linear"), rtc.Device(BASE + ",mb_bounds=swept")
    log = []
    fn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda user, code, msg: log.append((code, (msg or b"").decode())))
    d0.lib.rtcSetDeviceErrorFunction(d0.handle, C.cast(fn, C.c_void_p), None)
    v, t = random_soup(16, 1)
    other = rtc.Scene(d1)
    other.add_triangles_mb([v, (v + np.float32(0.25)).astype(np.float32)], t)
    other.commit()
    top = rtc.Scene(d0)
    g = top.lib.rtcNewGeometry(d0.handle, rtc.RTC_GEOMETRY_TYPE_INSTANCE)
    top.lib.rtcSetGeometryInstancedScene(g, other.handle)
    assert d0.error() == rtc.RTC_ERROR_INVALID_OPERATION
    assert log and log[-1][0] == rtc.RTC_ERROR_INVALID_OPERATION and "inputs are from different devices" in log[-1][1], log
    top.lib.rtcReleaseGeometry(g)
    top.release()
    other.release()
    d0.release()
    d1.release()
