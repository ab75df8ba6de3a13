"""Shared by tests/test_host_instance_hair_mb.py and tests/test_gpu_instance_hair_mb.py: instanced scenes that hold line segments and flat
curves WITH TIME STEPS (device config inst_hair=1,inst_hair_mb=1), alone or beside static hair and triangle and quad meshes - the kinds
22 / 23 with the HAIRMB form of the two-level kernel (embree-compressed_amd/csrc/trace_instance_hair_mb.hip).

An instanced scene is described as instance_hair_helpers describes one, with two more entries:
    {..., "curves_mb": [([verts4 per step], first_index, basis, tessellation rate, geomID), ...] or None,
          "lines_mb": ([verts4 per step], first_index, geomID) or None}

The layout (csrc/accel.h InstanceRecord / InstanceSceneRecord): `blobs` = the layout of instance_hair_helpers, then zero padding to a
multiple of 160 bytes and every scene's CurveMBRecords, then zero padding to a multiple of 80 bytes and every scene's LineMBRecords; a
scene record holds eight roots - words 0..3 the mesh trees, 4 and 5 the curve and the line tree, 6 and 7 the motion-blur curve and line
tree.  Visiting order is the slot order of a scene: triangles, motion-blur triangles, quads, motion-blur quads, curves, motion-blur
curves, lines, motion-blur lines."""
import numpy as np

import curve_helpers as ch
import curve_mb_helpers as cmb
import deep_stack_helpers as ds
import instance_hair_helpers as ihh
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
import line_helpers as lh
import line_mb_helpers as lmb
from instance_helpers import EMPTY, LEAF

HOST_CFG = ihh.HOST_CFG + ",quad_accel_mb=default,line_accel_mb=default,hair_accel_mb=default,inst_hair_mb=1"
GPU_CFG = "inst_hair=1,inst_hair_mb=1"
SCENE_DT = np.dtype([("triRoot", "<u4"), ("triMBRoot", "<u4"), ("quadRoot", "<u4"), ("quadMBRoot", "<u4"), ("curveRoot", "<u4"), ("lineRoot", "<u4"),
                     ("curveMBRoot", "<u4"), ("lineMBRoot", "<u4"), ("pad", "<u4", 8)])
assert SCENE_DT.itemsize == 64
TREE_CURVEMB, TREE_LINEMB = 6, 7
VISIT = imm.VISIT + (("curveRoot", ihh.TREE_CURVE), ("curveMBRoot", TREE_CURVEMB), ("lineRoot", ihh.TREE_LINE), ("lineMBRoot", TREE_LINEMB))
PART_OF = {"triRoot": "tris", "triMBRoot": "tris_mb", "quadRoot": "quads", "quadMBRoot": "quads_mb", "curveRoot": "curves", "curveMBRoot": "curves_mb",
           "lineRoot": "lines", "lineMBRoot": "lines_mb"}
F32 = np.float32
REFUSE_MB_LINEAR = "inst_hair_mb=1: motion blur line segments and flat curves below an instance are traced over swept boxes only; not under mb_bounds=linear"


def desc(tris=None, quads=None, tris_mb=None, quads_mb=None, curves=None, lines=None, curves_mb=None, lines_mb=None):
    d = ihh.desc(tris, quads, tris_mb, quads_mb, curves, lines)
    d["curves_mb"], d["lines_mb"] = curves_mb, lines_mb
    return d


# ---- geometry: vertices, radii and per-step offsets on the 2^-10 grid ------------------------------------------------------------------------
def snap4(v):
    return ih.snap(v)  # all four components: the radius is interpolated like a coordinate


def moving_steps(v, nsteps, seed, amount=0.5):
    """nsteps copies of verts4 `v` on the grid; step j > 0 moves every vertex by an offset of its own on the grid, radii included"""
    rng = np.random.default_rng(seed)
    v0 = snap4(v)
    steps = [v0]
    for j in range(1, nsteps):
        off = rng.uniform(-amount, amount, v0.shape)
        off[:, 3] *= 0.1
        s = snap4(steps[-1].astype(np.float64) + off)
        s[:, 3] = np.maximum(s[:, 3], F32(16.0 / 1024.0))
        steps.append(s)
    return steps


def moving_strands(nsteps=2, n_strands=12, per=8, seed=3, gid=0):
    v, idx = ihh.strands(n_strands, per, seed)
    return (moving_steps(v, nsteps, seed + 100), idx, gid)


def moving_curve_geometries(nsteps=3, first_gid=0, n=6, seed=10, combos=(("bezier", 1), ("bspline", 16), ("bspline", 4), ("bezier", 9))):
    """one geometry per (basis, tessellation rate): both bases, the rates 1 and 16 among them (rates above 8 take the leaf's second pass)"""
    out = []
    for k, (basis, rate) in enumerate(combos):
        v, idx = ihh.tuft(n, seed + k)
        out.append((moving_steps(v, nsteps, seed + 200 + k), idx, basis, rate, first_gid + k))
    return out


def still_copy(v, nsteps=2):
    """a moving geometry whose steps all equal `v` (on the grid): at times k / 8 lerp is exact and the geometry is `v`, bit for bit"""
    v0 = snap4(v)
    return [v0.copy() for _ in range(nsteps)]


def scenes(which):
    """the inner scenes of the short-ray leg: (a) 12 x 8 two-step lines, (b) 24 three-step curves, (c) all eight trees, (d) ties - a static
    and a still two-step geometry on the same vertices, the moving one with the higher geomID, for lines and for curves"""
    if which == "a":
        return {"m": desc(lines_mb=moving_strands(2))}
    if which == "b":
        return {"m": desc(curves_mb=moving_curve_geometries(3))}
    if which == "c":
        t, q = ihh.coincident_meshes(gid_tris=0, gid_quads=1)
        qv = [np.asarray(q[0], F32), ih.snap(np.asarray(q[0], np.float64) + np.array([0.25, 0.5, -0.125]))]
        sv, sidx = ihh.strands(6, 6, seed=13)
        regid = lambda gs, first: [g[:-1] + (first + k,) for k, g in enumerate(gs)]  # noqa: E731
        return {"m": desc(tris=t, quads=q, tris_mb=ihh.moving_triangles(gid=2, n=24), quads_mb=(qv, q[1], 3),
                          curves=regid(ihh.curve_geometries(n=6)[3:5], 4), curves_mb=regid(moving_curve_geometries(2, n=6)[1:3], 6),
                          lines=(snap4(sv), sidx, 8), lines_mb=moving_strands(2, 8, 6, seed=5, gid=9))}
    if which == "d":
        lv, lidx = ihh.strands(8, 6, seed=7, radius=(0.25, 0.5))
        cv, cidx = ihh.tuft(12, seed=8, radius=(0.25, 0.5))
        return {"m": desc(lines=(snap4(lv), lidx, 0), lines_mb=(still_copy(lv), lidx, 1),
                          curves=[(snap4(cv), cidx, "bezier", 4, 2)], curves_mb=[(still_copy(cv), cidx, "bezier", 4, 3)])}
    raise KeyError(which)


def moving_gids(d):
    return [g[4] for g in (d.get("curves_mb") or [])] + ([d["lines_mb"][2]] if d.get("lines_mb") is not None else [])


def points(d):
    """every point of a scene description at every time step, the radii added on all sides"""
    static = {k: d.get(k) for k in ("tris", "quads", "tris_mb", "quads_mb", "curves", "lines")}
    out = [ihh.points(static)] if any(v is not None for v in static.values()) else []
    hair = list(d.get("curves_mb") or []) + ([d["lines_mb"]] if d.get("lines_mb") is not None else [])
    for g in hair:
        for s in g[0]:
            v = np.asarray(s, np.float64).reshape(-1, 4)
            r = np.abs(v[:, 3]).max()
            out += [v[:, :3] - r, v[:, :3] + r]
    return np.concatenate(out)


def bounds_meshes(scs):
    return {k: (points(d),) for k, d in scs.items()}


# ---- building ---------------------------------------------------------------------------------------------------------------------------
def add_scene(rtc, dev, d, mode):
    sc = rtc.Scene(dev, iq.flags(mode))
    for part, add in (("tris", sc.add_triangles), ("tris_mb", sc.add_triangles_mb), ("quads", sc.add_quads), ("quads_mb", sc.add_quads_mb)):
        if d.get(part) is not None:
            v, idx, gid = d[part]
            assert add(v, idx, geom_id=gid) == gid
    for v, idx, basis, rate, gid in (d.get("curves") or []):
        assert sc.add_curves(v, idx, basis=basis, tessellation_rate=rate, geom_id=gid) == gid
    for steps, idx, basis, rate, gid in (d.get("curves_mb") or []):
        assert sc.add_curves_mb(steps, idx, basis=basis, tessellation_rate=rate, geom_id=gid) == gid
    if d.get("lines") is not None:
        v, idx, gid = d["lines"]
        assert sc.add_lines(v, idx, geom_id=gid) == gid
    if d.get("lines_mb") is not None:
        steps, idx, gid = d["lines_mb"]
        assert sc.add_lines_mb(steps, idx, geom_id=gid) == gid
    sc.commit()
    return sc


def build(rtc, mode, scs, instances, cfg=GPU_CFG, extra=None, commit=True):
    dev = rtc.Device(cfg)
    inner = {k: add_scene(rtc, dev, d, mode) for k, d in scs.items()}
    top = rtc.Scene(dev, iq.flags(mode))
    for gid, key, steps in instances:
        if len(steps) == 1:
            assert top.add_instance(inner[key], steps[0], geom_id=gid) == gid
        else:
            assert top.add_instance_mb(inner[key], steps, geom_id=gid) == gid
    keep = extra(top, dev) if extra else None
    if commit:
        top.commit()
    top._extra_keep = keep
    return dev, top, inner


release = ihh.release


# ---- decoding the accel -------------------------------------------------------------------------------------------------------------------
def split_blobs(blobs, n_inst, n_quads, n_steps, n_scenes, n_trimb, n_quadmb, n_curves, n_lines, n_curvemb, n_linemb):
    """the sections of `blobs` of an accel with moving hair: dict of the record arrays and of the byte offsets "curvemb_off", "linemb_off";
    asserts alignment, zero padding and the total size"""
    o = 64 * (n_inst + n_quads + n_steps + n_scenes)
    out = {"recs": blobs[: 64 * n_inst].view(ih.INST_DT), "quads": blobs[64 * n_inst: 64 * (n_inst + n_quads)].view(iq.QUAD_DT),
           "steps": blobs[64 * (n_inst + n_quads): 64 * (n_inst + n_quads + n_steps)].view(im.STEP_DT), "scenes": blobs[o - 64 * n_scenes: o].view(SCENE_DT)}
    for name, dt, n in (("trimb", ds.TRIMB_DT, n_trimb), ("quadmb", ds.QUADMB_DT, n_quadmb), ("curves", ch.CURVE_DT, n_curves), ("lines", lh.LINE_DT, n_lines),
                        ("curvemb", cmb.CURVEMB_DT, n_curvemb), ("linemb", lmb.LINEMB_DT, n_linemb)):
        size = dt.itemsize
        off = (o + size - 1) // size * size
        assert not blobs[o:off].any() and off % size == 0
        out[name], out[name + "_off"] = blobs[off: off + size * n].view(dt), off
        o = off + size * n
    assert o == len(blobs), (o, len(blobs))
    return out


def own_hair_mb(rtc, d, mode, cfg=HOST_CFG):
    """{"curves_mb" / "lines_mb": (nodes, records, root, maxDepth, kind) or None}: the moving-hair accels of `d` as scenes of their own"""
    dev = rtc.Device(cfg)
    out = {}
    for part, dt in (("curves_mb", cmb.CURVEMB_DT), ("lines_mb", lmb.LINEMB_DT)):
        if d.get(part) is None:
            out[part] = None
            continue
        sc = add_scene(rtc, dev, desc(**{part: d[part]}), mode)
        out[part] = (sc.accel_data(0).view(ih.NODE_DT).copy(), sc.accel_data(2).view(dt).copy(), sc.accel_root(), sc.stats()["maxDepth"], sc.stats()["accelKind"])
        sc.release()
    dev.release()
    return out


def own_hair(rtc, d, mode, cfg=HOST_CFG):
    """{"curves" / "lines": (nodes, records, root, maxDepth, kind) or None}: the static hair accels of `d` as scenes of their own"""
    dev = rtc.Device(cfg)
    out = {}
    for part, dt in (("curves", ch.CURVE_DT), ("lines", lh.LINE_DT)):
        if d.get(part) is None:
            out[part] = None
            continue
        sc = ihh.add_scene(rtc, dev, ihh.desc(**{part: d[part]}), mode)
        out[part] = (sc.accel_data(0).view(ih.NODE_DT).copy(), sc.accel_data(2).view(dt).copy(), sc.accel_root(), sc.stats()["maxDepth"], sc.stats()["accelKind"])
        sc.release()
    dev.release()
    return out


def scene_roots(blobs, inst_record):
    """the eight roots of the instance's scene record in VISITING order: [(name, code, root)]"""
    words = blobs.view(np.uint32)
    base = int(inst_record["root"]) * 16
    sc = words[base: base + 16].view(SCENE_DT)[0]
    return [(name, code, int(sc[name])) for name, code in VISIT]


# ---- the stack walk of a ray that hits nothing (static instances) --------------------------------------------------------------------------
def simulate_stack(nodes, root, blobs, n_inst, org, dirs):
    """instance_hair_helpers.simulate_stack for eight roots per scene record: entering an instance stacks the exit marker and, in reverse
    visiting order, one marker per pending tree (its code with its root).  Returns (deepest slot written per ray, per ray the list of
    (instance geomID, [tree codes in the order the walk continued in them]))."""
    lo, hi, child = ds.decode_nodes(nodes)
    recs = blobs[: 64 * n_inst].view(ih.INST_DT)
    out, visits = [], []
    for i in range(len(org)):
        wo, wd = np.asarray(org[i], np.float64), np.asarray(dirs[i], np.float64)
        o, d = wo, wd
        stack, deepest, cur, seen = [], -1, int(root), []
        while True:
            if cur != EMPTY and not (cur & LEAF):
                with np.errstate(divide="ignore", invalid="ignore"):
                    t1, t2 = (lo[cur] - o) / d, (hi[cur] - o) / d
                tn = np.fmax(np.minimum(t1, t2).max(1), 0.0)
                tf = np.maximum(t1, t2).min(1)
                hits = [(tn[k], -k, int(child[cur][k])) for k in range(8) if int(child[cur][k]) != EMPTY and tn[k] <= tf[k]]
                hits.sort()
                if hits:
                    for h in reversed(hits[1:]):
                        stack.append(h[2])
                        deepest = max(deepest, len(stack) - 1)
                    cur = hits[0][2]
                    continue
            elif cur != EMPTY and o is wo and (cur & LEAF) and ((cur >> 26) & 31):  # an instance leaf of the top level
                r = recs[cur & 0x3FFFFFF]
                m = r["world2local"].astype(np.float64).reshape(4, 3)
                o, d = wo @ m[:3] + m[3], wd @ m[:3]
                stack.append(imm.REF_INST_EXIT)
                have = [(code, x) for _, code, x in scene_roots(blobs, r) if x != EMPTY]
                for code, x in reversed(have[1:]):
                    stack.append(("tree", code, x))  # the marker REF_INST_TREE(code) with the root in its distance word
                deepest = max(deepest, len(stack) - 1)
                seen.append((int(r["geomID"]), [have[0][0]] if have else []))
                cur = have[0][1] if have else EMPTY
                continue
            if not stack:
                break
            cur = stack.pop()
            if isinstance(cur, tuple):
                seen[-1][1].append(cur[1])
                cur = cur[2]
            elif cur == imm.REF_INST_EXIT:
                o, d = wo, wd
                cur = EMPTY
        out.append(deepest)
        visits.append(seen)
    return np.array(out), visits


# ---- the float64 truth of the general-transform leg ---------------------------------------------------------------------------------------
def steps_at64(steps, time):
    """the float32 step arrays interpolated in float64 at `time` (getTimeSegment: times outside [0, 1] extrapolate)"""
    it, f = lmb.time_segment64(time, len(steps) - 1)
    return (1.0 - f) * np.asarray(steps[it], np.float64) + f * np.asarray(steps[it + 1], np.float64)
