"""What the tests of the linear-bounds motion-blur accels (device config mb_bounds=linear) share: the QNodeMB8 record, its decode at a
ray time with the kernel's arithmetic, the kernel's record selection and vertex interpolation, the scenes, and a host simulation of the
traversal stack over the new nodes."""
import numpy as np

NODEMB_DT = np.dtype([("origin", "<f4", 3), ("exp", "u1", 3), ("pad", "u1"), ("child", "<u4", 8), ("q", "u1", (6, 8)), ("q1", "u1", (6, 8))])
NODE_DT = np.dtype([("origin", "<f4", 3), ("exp", "u1", 3), ("pad", "u1"), ("child", "<u4", 8), ("q", "u1", (6, 8))])
TRIMB_DT = np.dtype([("a0", "<f4", 3), ("geomID", "<u4"), ("b0", "<f4", 3), ("primID", "<u4"), ("c0", "<f4", 3), ("segment", "<u4"),
                     ("a1", "<f4", 3), ("numSegments", "<u4"), ("b1", "<f4", 3), ("pad0", "<u4"), ("c1", "<f4", 3), ("pad1", "<u4")])
QUADMB_DT = np.dtype([("v0a", "<f4", 3), ("pad0", "<u4"), ("v1a", "<f4", 3), ("primID", "<u4"), ("v2a", "<f4", 3), ("pad1", "<u4"),
                      ("v3a", "<f4", 3), ("geomID", "<u4"), ("v0b", "<f4", 3), ("pad2", "<u4"), ("v1b", "<f4", 3), ("segment", "<u4"),
                      ("v2b", "<f4", 3), ("pad3", "<u4"), ("v3b", "<f4", 3), ("numSegments", "<u4")])
TRI_ENDS = (("a0", "b0", "c0"), ("a1", "b1", "c1"))
QUAD_ENDS = (("v0a", "v1a", "v2a", "v3a"), ("v0b", "v1b", "v2b", "v3b"))
assert NODEMB_DT.itemsize == 144 and NODE_DT.itemsize == 96
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST
# the builder's documented guarantee (csrc/accel.h QNodeMB8): at t = 0 and t = 1 every decoded plane lies at least one and less than
# two steps of its node's grid outside the exact bounds of the records below
PAD_STEPS = 2.0


def fma32(a, b, c):
    """fmaf on float32 arrays: product and sum in float64 (exact for the operands of these tests), one rounding to float32"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64) + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def scales(node):
    return (node["exp"].astype(np.uint32) << 23).view(np.float32)


def decode_children_mb(node, t):
    """(lo[8, 3], hi[8, 3]) of the eight children of a QNodeMB8 at ray time t, with the node step's arithmetic:
    tc = min(max(t, 0), 1); plane = fmaf(fmaf(tc, float(q1) - float(q0), float(q0)), scale, origin)"""
    tc = np.fmin(np.fmax(np.float32(t), np.float32(0)), np.float32(1))  # fmaxf / fminf: a NaN time becomes 0
    q0, q1 = node["q"].astype(np.float32), node["q1"].astype(np.float32)  # [6, 8]
    qf = fma32(tc, q1 - q0, q0)
    s, o = np.repeat(scales(node), 2)[:, None], np.repeat(node["origin"], 2)[:, None]
    p = fma32(qf, s, o)  # [6, 8]
    return p[0::2].T.copy(), p[1::2].T.copy()


def time_segment(time, num_segments):
    """(itime, ftime) of trace_mb.hip.h time_segment in float32"""
    S = np.float32(num_segments)
    ts = np.float32(np.float32(time) * S)
    it = np.float32(min(max(np.floor(ts), np.float32(0)), S - np.float32(1)))
    return int(it), np.float32(ts - it)


def lerp_vertex(p0, p1, f):
    """trace_mb.hip.h lerp_vertex: fmaf(1 - f, p0, f * p1) in float32"""
    f = np.float32(f)
    g = np.float32(np.float32(1) - f)
    return fma32(g, p0, (f * np.asarray(p1, np.float32)).astype(np.float32))


def record_vertices(rec, ends, time):
    """the vertices [nv, 3] record `rec` produces for a ray at `time`, or None when the record does not accept that time"""
    it, f = time_segment(time, int(rec["numSegments"]))
    if it != int(rec["segment"]):
        return None
    return np.stack([lerp_vertex(rec[a], rec[b], f) for a, b in zip(*ends)])


def walk_paths(nodes, root):
    """yields (path, first, count) for every leaf: path = [(node index, child slot), ...] from the root down"""
    if root & LEAF:
        yield [], root & 0x3FFFFFF, (root >> 26) & 31
        return
    todo = [(root, [])]
    while todo:
        n, path = todo.pop()
        for i, c in enumerate(nodes[n]["child"]):
            c = int(c)
            if c == EMPTY:
                continue
            if c & LEAF:
                yield path + [(n, i)], c & 0x3FFFFFF, (c >> 26) & 31
            else:
                todo.append((c, path + [(n, i)]))


def snap(v, limit=64):
    s = np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0
    assert np.abs(s).max() < limit
    return s.astype(np.float32)


def rot_y(v, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    m = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    ctr = (v.min(0) + v.max(0)) / 2
    return (np.asarray(v, np.float64) - ctr) @ m.T + ctr


SCALE = 0.0625  # the bomberman spans +-246: below 64 in every (moved) step, as in test_gpu_motion_blur.py


def bomberman_two_steps(v):
    """the moved 2-step bomberman of test_gpu_motion_blur.py `two_steps` (scene (a) of docs/experiments.md "Motion blur")"""
    s0 = snap(v * SCALE)
    ext = s0.max(0) - s0.min(0)
    return [s0, snap(rot_y(s0, 20.0) + np.array([0.3 * ext[0], 0.0, 0.0]))]


def bomberman_five_steps(v):
    s0 = snap(v * SCALE)
    ext = s0.max(0) - s0.min(0)
    return [snap(rot_y(s0, 12.0 * k) + ext * np.array([0.1 * k, 0.03 * k * k, -0.05 * k])) for k in range(5)]


def grid_tris(n=8):
    """(n+1)^2 vertices of a warped grid (the grid of test_host_motion_blur.py, snapped to multiples of 2^-10), 2 n^2 triangles"""
    xs, ys = np.meshgrid(np.arange(n + 1, dtype=np.float32), np.arange(n + 1, dtype=np.float32))
    v = snap(np.stack([xs.ravel(), ys.ravel(), (0.3 * np.sin(xs) * np.cos(ys)).ravel()], 1))
    t = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            t += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    return v, np.array(t, np.uint32)


def grid_quads(n=8):
    v, _ = grid_tris(n)
    q = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            q.append((a, a + 1, a + n + 2, a + n + 1))
    return v, np.array(q, np.uint32)


def curved_steps(v, nsteps):
    """nsteps time steps on a curved path: a rotation about y and a parabola (as five_steps), snapped"""
    ext = v.max(0) - v.min(0)
    return [snap(rot_y(v, 12.0 * k) + ext * np.array([0.1 * k, 0.03 * k * k, -0.05 * k])) for k in range(nsteps)]


# ---- host simulation of the traversal stack over QNodeMB8 nodes -----------------------------------------------------------------
def decode_nodes_mb(nodes, time):
    """child boxes of every QNodeMB8 at ray time `time` as the node step decodes them (decode_children_mb, vectorised over the nodes):
    (lo [N, 8, 3], hi [N, 8, 3]) float64 and the children [N][8] as Python ints - the form deep_stack_helpers walks"""
    tc = np.fmin(np.fmax(np.float32(time), np.float32(0)), np.float32(1))
    q0, q1 = nodes["q"].astype(np.float32), nodes["q1"].astype(np.float32)  # [N, 6, 8]
    qf = fma32(tc, q1 - q0, q0)
    s = np.repeat((nodes["exp"].astype(np.uint32) << 23).view(np.float32), 2, axis=1)[:, :, None]
    o = np.repeat(nodes["origin"], 2, axis=1)[:, :, None]
    p = fma32(qf, s, o).astype(np.float64)
    return np.ascontiguousarray(p[:, 0::2].transpose(0, 2, 1)), np.ascontiguousarray(p[:, 1::2].transpose(0, 2, 1)), nodes["child"].tolist()


def simulate_stack_mb(nodes, root, leaves, org, dirs, times, threshold=16):
    """deep_stack_helpers.simulate_stack over time-dependent nodes: every ray walks the boxes decoded at its own time.  Returns the
    highest stack slot every ray wrote (-1: none)."""
    import deep_stack_helpers as ds
    org, dirs = np.asarray(org, np.float64), np.asarray(dirs, np.float64)
    times = np.asarray(times, np.float32)
    deepest = np.full(len(org), -1, np.int64)
    for t in np.unique(times):
        lo, hi, child = decode_nodes_mb(nodes, t)
        for i in np.nonzero(times == t)[0]:
            deepest[i] = ds._walk_one(lo, hi, child, int(root), leaves, org[i], dirs[i], 0.0, float("inf"), float(t), threshold, None).deepest
    return deepest
