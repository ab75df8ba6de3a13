"""Shared by tests/test_host_instance_subdiv_top_linear.py and tests/test_gpu_instance_subdiv_top_linear.py: moving instances of
subdivision scenes under time-dependent top-level boxes (device config inst_subdiv_bounds=linear; accel kinds 34 / 35).

The accel (embree-compressed_amd/csrc/accel.h, InstanceRecord): `blobs` is the layout of the kinds 24 / 25 (InstanceRecords |
InstanceSteps | padding | leaf blobs); the node buffer has two sections, the instanced scenes' BVH8s as QNode8s from its start, zero
padding to a multiple of 144 bytes, then the top-level tree as QNodeMB8s.  The root and the inner references of the top-level tree
index the buffer as one array of QNodeMB8; blobOffsets has four words (leaf blobs, first blob, QNodeMB8s, first QNodeMB8).

Meshes and instances are described as in instance_subdiv_helpers; the motion patterns are instance_top_linear_helpers.instances("a".."e")
over one instanced scene "m" that fills about [0, 10]^3 as the soup those patterns were made for does."""
import numpy as np

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_subdiv_helpers as isd
import instance_top_linear_helpers as itl
from instance_helpers import EMPTY, LEAF
from mb_linear_helpers import NODEMB_DT, decode_nodes_mb, walk_paths

ACCEL_INSTSUBDIV_TOP_LINEAR_GRID, ACCEL_INSTSUBDIV_TOP_LINEAR_CBVH_LEAF = 34, 35
KIND = {isd.EAGER: ACCEL_INSTSUBDIV_TOP_LINEAR_GRID, isd.LEAF: ACCEL_INSTSUBDIV_TOP_LINEAR_CBVH_LEAF}
KEY = "inst_subdiv_bounds=linear"
HOST = "gpu=none,inst_accel=default"
HOST_KEY = HOST + "," + KEY
REF_INST_EXIT = ds.REF_INST_EXIT
F32 = np.float32


def big_cube(L=4, C=2):
    """instance_subdiv_helpers.cube() scaled by four and moved to [1, 9]^3 (exact on the 2^-10 grid): the size of the scene the motion
    patterns of instance_top_linear_helpers.instances() were made for"""
    v, fs, fi = isd.cube()
    return (v * F32(4) + F32(5)).astype(F32), fs, fi, L, C


def build_pair(rtc, accel, meshes, inst, cfg=""):
    """the same scene on a device without the key (swept) and on one with it: ((dev, top, inner) swept, (dev, top, inner) linear)"""
    swept = isd.build(rtc, accel, meshes, inst, cfg)
    lin = isd.build(rtc, accel, meshes, inst, (cfg + "," if cfg else "") + KEY)
    return swept, lin


# ---- the exported accel -----------------------------------------------------------------------------------------------------------------------
def split_nodes(top, rtc):
    """(QNode8 section, the buffer as ONE array of QNodeMB8, number of QNodeMB8s, index of the first one, (leaf blobs, first blob)) of
    a subdivision instance accel of kind 34 / 35; asserts the sizes, the zero padding and that the statistics describe the QNode8s"""
    sel = rtc.ACCEL_DATA_INSTSUBDIV
    image = top.accel_data(sel + 0)
    off = top.accel_data(sel + 3).view(np.uint32)
    assert len(off) == 4, len(off)
    nblobs, first_blob, n_mb, first = (int(x) for x in off)
    st = top.stats()  # (a top scene that holds nothing but subdivision instances exports this accel)
    assert st["nodeBytes"] == 96
    n8 = st["nodeCount"]
    assert first == (n8 * 96 + 143) // 144, (n8, first)
    assert len(image) == (first + n_mb) * 144, (len(image), first, n_mb)
    assert not image[n8 * 96:first * 144].any()  # the padding
    return image[:n8 * 96].view(ih.NODE_DT), image.view(NODEMB_DT), n_mb, first, (nblobs, first_blob)


def top_leaves(top, rtc):
    """(image_mb, [(path, record index)]) of the top-level tree: path = [(QNodeMB8 index in 144-byte units, child slot), ...]"""
    _, image_mb, n_mb, first, _ = split_nodes(top, rtc)
    root = top.accel_root()
    assert not root & LEAF and first <= root < first + n_mb  # an inner node of the second section, even for a single instance
    out = []
    for path, rec, n in walk_paths(image_mb, root):
        assert n == 1 and all(first <= node < first + n_mb for node, _ in path)
        out.append((path, rec))
    return image_mb, out


def records(top, rtc, n):
    return top.accel_data(rtc.ACCEL_DATA_INSTSUBDIV + 2)[:64 * n].view(ih.INST_DT)


# ---- the stack walk: QNodeMB8s outside an instance, QNode8s inside, no leaf tests (the walk of a ray that hits nothing) -----------------------------
def simulate_stack(top, rtc, n_inst, org, dirs, times):
    """per ray the deepest stack slot written (-1: none).  A moving instance is entered through the float64 inverse of its lerped steps."""
    nodes8, image_mb, _, _, _ = split_nodes(top, rtc)
    static = ds.decode_nodes(nodes8)
    blobs = top.accel_data(rtc.ACCEL_DATA_INSTSUBDIV + 2)
    recs, blobs64 = blobs[:64 * n_inst].view(ih.INST_DT), blobs.view(np.uint8)
    times = np.asarray(times, F32)
    out = np.zeros(len(org), np.int64)
    for t in np.unique(times):
        with np.errstate(over="ignore", invalid="ignore"):  # entries that overlay QNode8s decode to anything: no QNodeMB8 reference names them
            timed = decode_nodes_mb(image_mb, t)
        for i in np.nonzero(times == t)[0]:
            out[i] = _walk_one(static, timed, int(top.accel_root()), np.asarray(org[i], np.float64), np.asarray(dirs[i], np.float64), float(t), recs, blobs64)
    return out


def _entry_matrix(rec, blobs, time):
    pad1 = int(rec["pad"][1])
    if pad1 == 0:
        return rec["world2local"].astype(np.float64).reshape(4, 3)
    S, first = pad1 >> 24, pad1 & 0xFFFFFF
    steps = blobs[64 * first:64 * (first + S + 1)].view(im.STEP_DT)["local2world"].reshape(-1, 4, 3).transpose(0, 2, 1)
    return np.ascontiguousarray(im.world2local_f64(steps, np.array([time], F32))[0].T)


def _walk_one(static, timed, root, wo, wd, time, recs, blobs):
    o, d = wo, wd
    with np.errstate(divide="ignore"):
        rd = 1.0 / d
    stack, deepest = [], -1
    cur, inside = root, False
    while True:
        if cur != EMPTY and not cur & LEAF:
            lo, hi, child = static if inside else timed
            with np.errstate(invalid="ignore"):
                t1, t2 = (lo[cur] - o) * rd, (hi[cur] - o) * rd
            tn = np.maximum(np.minimum(t1, t2).max(1), 0.0)
            tf = np.maximum(t1, t2).min(1)
            ch = child[cur]
            ks = [k for k in np.nonzero(tn <= tf)[0].tolist() if ch[k] != EMPTY]
            if not ks:
                cur = EMPTY
            elif len(ks) == 1:
                cur = ch[ks[0]]
            else:
                order = ds._order(ks, [float(tn[k]) for k in ks])
                cur = ch[order[0]]
                for k in reversed(order[1:]):
                    stack.append(ch[k])
                deepest = max(deepest, len(stack) - 1)
            if cur != EMPTY:
                continue
        elif cur != EMPTY and not inside:
            rec = recs[cur & 0x3FFFFFF]
            m = _entry_matrix(rec, blobs, time)
            o, d = wo @ m[:3] + m[3], wd @ m[:3]
            with np.errstate(divide="ignore"):
                rd = 1.0 / d
            stack.append(REF_INST_EXIT)
            deepest = max(deepest, len(stack) - 1)
            inside = True
            cur = int(rec["root"])
            if cur != EMPTY:
                continue
        cur = EMPTY  # (a subdivision leaf: not tested)
        while stack:
            ref = stack.pop()
            if ref == REF_INST_EXIT:
                o, d, inside = wo, wd, False
                with np.errstate(divide="ignore"):
                    rd = 1.0 / d
                continue
            cur = ref
            break
        if cur == EMPTY:
            return deepest


# ---- the deep case: the needle patches of test_gpu_instance_subdiv_deep_stack.py under moving instances --------------------------------------------
N_NEEDLES, WIDTH = 1024, 0.004


def needle_meshes():
    v, q = ds.sliver_soup(N_NEEDLES, ds.SOUP_SEED, quads=True, snapped=True, width=WIDTH)
    return {"m": (v, np.full(N_NEEDLES, 4, np.uint32), q.reshape(-1).astype(np.uint32), 1, 1)}


def deep_moving_instances():
    """deep_stack_helpers.deep_instances() with a second step each: the same linear part, the translation moved by a few 2^-4 steps, so
    that world2local(time) stays exact at the times k / 4 and the three boxes keep overlapping over the whole shutter"""
    out = []
    for (g, k, m), move in zip(ds.deep_instances(), ((0.125, 0.0, -0.0625), (-0.125, 0.0625, 0.0), (0.0, -0.0625, 0.125))):
        m1 = np.array(m, F32)
        m1[:, 3] += np.asarray(move, F32)
        out.append((g, k, [m, m1]))
    return out


def chain_instances(n=24):
    """nested moving instances of the needle mesh: instance i is the mesh scaled by 1 + i / 32 about the centre of the unit cube, every
    one with a second step moved by 1 / 16 along x - box i lies inside box i + 1 at every time, a ray through the middle enters all"""
    out = []
    for i in range(n):
        s = 1.0 + i / 32.0
        t = 0.5 - 0.5 * s
        out.append((i, "m", [ih.affine((t, t, t), (s,) * 3), ih.affine((t + 0.0625, t, t), (s,) * 3)]))
    return out


def path_boxes(image_mb, path, t):
    return itl.path_boxes(image_mb, path, t)
