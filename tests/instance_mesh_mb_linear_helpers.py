"""Shared by tests/test_host_instance_mesh_mb_linear.py and tests/test_gpu_instance_mesh_mb_linear.py: instanced scenes whose motion-blur
accels keep their time-dependent nodes below the instance (device config mb_bounds=linear,inst_mb_bounds=linear; accel kinds 30 / 31).

The node buffer of such an accel (embree-compressed_amd/csrc/accel.h, InstanceRecord) has two sections: QNode8s (96 bytes: the top-level
tree and every scene's static triangle and quad trees) | zero padding up to a multiple of 144 bytes | QNodeMB8s (144 bytes: every scene's
motion-blur triangle and quad trees).  References inside a motion-blur tree index the buffer as ONE array of QNodeMB8.  `blobOffsets`
holds the number of QNodeMB8s and the index of the first, in 144-byte units; `blobs` and `prims` are those of the kinds 22 / 23."""
import numpy as np

import deep_stack_helpers as ds
import instance_mesh_mb_helpers as imm
from instance_helpers import EMPTY, LEAF, NODE_DT
from mb_linear_helpers import NODEMB_DT, decode_nodes_mb

ACCEL_INSTMESHMB_LINEAR_PLUECKER, ACCEL_INSTMESHMB_LINEAR_MOELLER = 30, 31
LINEAR = "mb_bounds=linear,inst_mb_bounds=linear"
REF_INST_EXIT = imm.REF_INST_EXIT
MB_CODES = (imm.TREE_TRIMB, imm.TREE_QUADMB)  # bit 1 of the code: a tree of QNodeMB8s


def kind(mode):
    """mode 0: Pluecker / robust, mode 1: Moeller / fast"""
    return ACCEL_INSTMESHMB_LINEAR_PLUECKER if mode == 0 else ACCEL_INSTMESHMB_LINEAR_MOELLER


def split_nodes(top):
    """(QNode8 section, the buffer as ONE array of QNodeMB8, number of QNodeMB8s, index of the first one) of a scene of kind 30 / 31;
    asserts the sizes, the zero padding and that the statistics describe the QNode8 section"""
    image = top.accel_data(0)
    n_mb, first = (int(x) for x in top.accel_data(3).view(np.uint32))
    st = top.stats()
    assert st["nodeBytes"] == 96
    n8 = st["nodeCount"]
    assert first == (n8 * 96 + 143) // 144, (n8, first)
    assert len(image) == (first + n_mb) * 144, (len(image), first, n_mb)
    assert not image[n8 * 96:first * 144].any()  # the padding
    return image[:n8 * 96].view(NODE_DT), image.view(NODEMB_DT), n_mb, first


# ---- the stack walk over both node types ------------------------------------------------------------------------------------------------------
def simulate_stack(top, org, dirs, times, inst, tfar=np.inf):
    """instance_mesh_mb_helpers.simulate_stack restated for the kinds 30 / 31: the same walk with the same markers, where a lane inside a
    motion-blur tree (codes TREE_TRIMB, TREE_QUADMB) reads its node from the buffer as an array of QNodeMB8 and decodes the children at
    the ray's time clamped to [0, 1] (mb_linear_helpers.decode_nodes_mb: the node step's arithmetic), every other lane reads a QNode8.
    Returns per ray (deepest slot written, most markers stacked at once, deepest slot written while at least one tree marker was on the
    stack, highest slot a tree marker itself was written to; -1: none)."""
    nodes8, image_mb, _, _ = split_nodes(top)
    static = ds.decode_nodes(nodes8)
    times = np.asarray(times, np.float32)
    out = np.zeros((len(org), 4), np.int64)
    for t in np.unique(times):
        with np.errstate(over="ignore", invalid="ignore"):  # entries that overlay QNode8s decode to anything: no motion-blur tree names them
            timed = decode_nodes_mb(image_mb, t)
        for i in np.nonzero(times == t)[0]:
            out[i] = _walk_one(static, timed, int(top.accel_root()), np.asarray(org[i], np.float64), np.asarray(dirs[i], np.float64), float(tfar), float(t), inst)
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]


def _walk_one(static, timed, root, wo, wd, tfar, time, inst):
    o, d = wo, wd
    with np.errstate(divide="ignore"):
        rd = 1.0 / d
    stack, deepest, most_markers, deepest_marked, marker_slot = [], -1, 0, -1, -1
    cur, inside, code = root, False, imm.TREE_TRI

    def note():
        nonlocal deepest, most_markers, deepest_marked
        deepest = max(deepest, len(stack) - 1)
        nm = sum(1 for r, _ in stack if REF_INST_EXIT < r <= REF_INST_EXIT + 3)
        most_markers = max(most_markers, nm)
        if nm:
            deepest_marked = max(deepest_marked, len(stack) - 1)

    if root == EMPTY:
        return -1, 0, -1, -1
    while True:
        if cur != EMPTY and not cur & LEAF:
            lo, hi, child = timed if inside and code in MB_CODES else static
            t1, t2 = (lo[cur] - o) * rd, (hi[cur] - o) * rd
            tn = np.maximum(np.minimum(t1, t2).max(1), 0.0)
            tf = np.minimum(np.maximum(t1, t2).min(1), tfar)
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
                    stack.append((ch[k], float(tn[k])))
                note()
            if cur != EMPTY:
                continue
        elif cur != EMPTY and not inside:
            rec = inst.records[cur & 0x3FFFFFF]
            m = rec["world2local"].astype(np.float64).reshape(4, 3)
            o, d = wo @ m[:3] + m[3], wd @ m[:3]
            with np.errstate(divide="ignore"):
                rd = 1.0 / d
            stack.append((REF_INST_EXIT, 0.0))
            inside = True
            sc = inst.scenes[int(rec["root"]) - inst.scene_base]
            have = [(int(sc[f]), c) for f, c in imm.VISIT if int(sc[f]) != EMPTY]
            for r, c in reversed(have[1:]):
                stack.append((imm.marker(c), r))
                marker_slot = max(marker_slot, len(stack) - 1)
            note()
            cur, code = have[0] if have else (EMPTY, imm.TREE_TRI)
            if cur != EMPTY:
                continue
        elif cur != EMPTY:
            t = ds._leaf_hit(inst.leaves[code], cur & 0x3FFFFFF, (cur >> 26) & 31, o, d, 0.0, tfar, time)
            if t is not None:
                tfar = t
        cur = EMPTY
        while stack:
            ref, dist = stack.pop()
            if ref == REF_INST_EXIT:
                o, d, inside, code = wo, wd, False, imm.TREE_TRI
                with np.errstate(divide="ignore"):
                    rd = 1.0 / d
                continue
            if REF_INST_EXIT < ref <= REF_INST_EXIT + 3:
                cur, code = int(dist), ref - REF_INST_EXIT
                break
            if dist > tfar:
                continue
            cur = ref
            break
        if cur == EMPTY:
            return deepest, most_markers, deepest_marked, marker_slot


# ---- the fast mover ---------------------------------------------------------------------------------------------------------------------------
FAST_N = 8  # the grid of mb_linear_helpers.grid_tris / grid_quads: 8 x 8 cells over [0, 8]^2, |z| <= 0.3
FAST_SHIFT = 16.0 * FAST_N  # between its two steps the mesh moves 16 x its extent along x
