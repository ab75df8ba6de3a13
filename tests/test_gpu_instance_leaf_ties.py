"""How a hit below an instance is attributed to its instance, leaf type by leaf type: the two-level kernels run the top-level mesh leaves
(TriLeaf, QuadLeaf, TriMBLeaf, QuadMBLeaf) on the local ray and give a hit the leaf commits the id of the instance being traversed.
One small scene per leaf type - one primitive, and a flat strip of 8 primitives in one plane - is placed by ONE instance and by TWO
instances with the same transform (twins: every candidate of one is a candidate of the other at a bit-identical t).  Everything but
instID must then be the bytes of the single instance, instID must be a twin's, the same one for 16-byte aligned records and for any
others (the kernels' VEC twins), and any-hit must end exactly the rays closest-hit ends.  Rays lie on the 2^-10 grid: on shared edges,
on the quads' diagonals, inside, and beside the strip."""
import ctypes as C

import numpy as np
import pytest

import instance_helpers as ih
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
from helpers import INVALID, fill_rays

pytestmark = pytest.mark.gpu

N = 64
FIELDS = ("tfar", "Ng_x", "Ng_y", "Ng_z", "u", "v", "geomID", "primID")
PLACE = ih.affine((0, 0, 1))
ONE, TWINS = (5,), (5, 9)
# accel kinds of the top-level scene (accel_kinds.h): static triangles 14 / 15, static quads 16 / 17, meshes with time steps 22 / 23
KIND = {"tris": 14, "quads": 16, "tris_mb": 22, "quads_mb": 22}


def _mesh(part, count):
    """`count` primitives in the plane z = 0 from x = 0 on: unit squares as quads, or halves of unit squares as triangles; with time steps
    the plane moves to z = 2 over the shutter.  Returns (scene description, extent in x)."""
    squares = count if part.startswith("quads") else (count + 1) // 2
    v = np.array([[x, y, 0] for x in range(squares + 1) for y in (0, 1)], np.float32)
    sq = [(2 * s, 2 * s + 2, 2 * s + 3, 2 * s + 1) for s in range(squares)]
    if part.startswith("quads"):
        idx = np.array(sq, np.uint32)
    else:
        idx = np.array([t for a, b, c, d in sq for t in ((a, b, c), (a, c, d))], np.uint32)[:count]
    assert len(idx) == count
    data = [v, v + np.array([0, 0, 2], np.float32)] if part.endswith("_mb") else v
    return imm.desc(**{part: (data, idx, 3)}), float(squares)


def _rays(rtc, width):
    """16 columns from x = 0 to the strip's end (its edges and, with y = 1/2, its diagonals among them) times 4 rows, the last beside it"""
    i = np.arange(N)
    x = (i % 16) * (width / 16.0)
    y = np.array([0.25, 0.5, 0.75, 1.25])[i // 16]
    rh = rtc.aligned_rayhits(N)
    fill_rays(rh, np.stack([x, y, np.full(N, -2.0)], 1).astype(np.float32), np.tile(np.array([0, 0, 1], np.float32), (N, 1)))
    rh["time"] = ((i % 9) / 8.0).astype(np.float32)
    return rh


def _unaligned(torch, recs):
    """the records in a device-resident array with a pitch of 96 bytes whose base is 4-byte aligned only: the kernels' VEC = false twins"""
    m, sz = len(recs), recs.dtype.itemsize
    raw = torch.zeros(m * 96 + 16, dtype=torch.uint8, device="cuda")
    view = raw[4:4 + m * 96].view(m, 96)
    assert view.data_ptr() % 16 == 4
    view[:, :sz] = torch.from_numpy(recs.view(np.uint8).reshape(m, sz).copy()).cuda()
    return view


def _trace(rtc, torch, dev, top, rays):
    """(closest hit aligned, closest hit unaligned, any hit aligned, any hit unaligned)"""
    out = []
    ctx = rtc.make_context()
    for recs, aligned_call, fn in ((iq.copy(rtc, rays), top.intersect1M, top.lib.rtcIntersect1M), (iq.occ_of(rtc, rays), top.occluded1M, top.lib.rtcOccluded1M)):
        view = _unaligned(torch, recs)
        fn(top.handle, C.byref(ctx), view.data_ptr(), len(recs), 96)
        dev.check("unaligned batch")
        torch.cuda.synchronize()
        aligned_call(recs)
        out += [recs, view[:, :recs.dtype.itemsize].contiguous().cpu().numpy().reshape(-1).view(recs.dtype)]
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("count", [1, 8])
@pytest.mark.parametrize("part", ["tris", "quads", "tris_mb", "quads_mb"])
def test_twin_instances_give_the_single_instances_hit_and_one_of_their_ids(rtc, part, count, mode):
    import torch
    d, width = _mesh(part, count)
    rays = _rays(rtc, width)
    dev = rtc.Device("")
    inner = imm.add_scene(rtc, dev, d, mode)
    got = {}
    for ids in (ONE, TWINS):
        top = rtc.Scene(dev, iq.flags(mode))
        for g in ids:
            assert top.add_instance(inner, PLACE, geom_id=g) == g
        top.commit()
        assert top.stats()["accelKind"] == KIND[part] + mode
        got[ids] = _trace(rtc, torch, dev, top, rays)
        top.release()
    inner.release()
    dev.release()
    want, want_u, wocc, wocc_u = got[ONE]
    hit = want["geomID"] != INVALID
    # the single instance: the plane is met at t = 3 (static) or 3 + 2 time, by every ray above the primitives, edges included with Pluecker
    assert 8 <= int(hit.sum()) <= 48 and not hit[48:].any() and (want["geomID"][hit] == 3).all() and (want["instID"][hit] == 5).all()
    moves = 2.0 if part.endswith("_mb") else 0.0
    assert np.array_equal(want["tfar"][hit], (3.0 + moves * rays["time"][hit]).astype(np.float32))
    assert want[~hit].tobytes() == rays[~hit].tobytes()
    assert want_u.tobytes() == want.tobytes() and wocc_u.tobytes() == wocc.tobytes()
    assert np.array_equal(wocc["tfar"] == -np.inf, hit) and np.array_equal(wocc["tfar"][~hit], rays["tfar"][~hit])
    two, two_u, occ, occ_u = got[TWINS]
    print(f"instID {part} x{count} mode {mode}: {' '.join('-' if g == INVALID else str(g) for g in two['instID'].tolist())}")
    for f in FIELDS:  # byte-equal to the same scene under one instance
        assert two[f].tobytes() == want[f].tobytes(), f
        assert two_u[f].tobytes() == want[f].tobytes(), f
    for rec in (two, two_u):
        assert np.isin(rec["instID"][hit], TWINS).all() and (rec["instID"][~hit] == INVALID).all()
        assert rec[~hit].tobytes() == rays[~hit].tobytes()
    assert np.array_equal(two["instID"], two_u["instID"])  # aligned and unaligned records: the same twin
    for o in (occ, occ_u):  # any hit ends the rays closest hit ends, and leaves the others as they were
        assert np.array_equal(o["tfar"] == -np.inf, hit) and np.array_equal(o["tfar"][~hit], rays["tfar"][~hit])
