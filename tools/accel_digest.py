"""Development check, CPU only: digest of what the seven primitive builders (csrc/rt_prim_build.cpp: triangles, quads, curves and lines,
static and with time steps) and the two instance builders (csrc/rt_instance_build.cpp) make of a fixed list of host-only scenes.  One line
per case: accel kind, root, every field of rtcamdGetSceneStats, rtcGetSceneBounds, and a SHA-256 per exported array (rtcamdGetAccelData
0..3 and 16..19); one line per refusal: error code and the full message; and the verbose=2 lines of one scene per record accel and of
the kinds 21, 23, 25 and 31 (printed by a child process, which this tool starts).  Run it once per library build (RTAMD_LIB=...) and
`diff` the listings: no difference = byte-identical accels, the same refusals.  The primitive scenes are generated here (sizes around the
leaf limits, skipped primitives, gaps in the geometry IDs, mixed time-step counts, every pair of types, recommits); the instance scenes
come from the helper modules of tests/.
usage: accel_digest.py > listing"""
import ctypes as C
import hashlib
import importlib
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

rtc = importlib.import_module('embree-compressed_amd').rtc
import instance_helpers as ih  # noqa: E402
import instance_mb_helpers as im  # noqa: E402
import instance_mesh_mb_helpers as imm  # noqa: E402
import instance_mesh_mb_linear_helpers as iml  # noqa: E402
import instance_quads_helpers as iq  # noqa: E402
import instance_subdiv_helpers as isd  # noqa: E402
from helpers import random_soup  # noqa: E402

d = np.load(os.path.join(ROOT, 'assets', 'bomberman.mesh.npz'))
BOMBERMAN = (d['verts'], d['face_sizes'], d['face_index'])
FULL = 'gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default'
LIN = FULL + ',' + iml.LINEAR
SUBDIV = 'gpu=none,inst_accel=default'
ARRAYS = (0, 1, 2, 3, 16, 17, 18, 19)
ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)


def digest(name, top):
    st = top.stats()
    lo, hi = top.bounds()
    arrays = ' '.join('%d:%s' % (k, hashlib.sha256(top.accel_data(k).tobytes()).hexdigest()[:20]) for k in ARRAYS)
    print('%s | kind %d root %08x | %s | bounds %s | %s' % (name, st['accelKind'], top.accel_root(), ' '.join('%s=%d' % kv for kv in st.items()),
                                                         ' '.join(float(x).hex() for x in (*lo, *hi)), arrays), flush=True)


def release(dev, top, inner):
    top.release()
    for s in inner.values():
        s.release()
    for s in (getattr(top, '_extra_keep', None) or []):
        s.release()
    dev.release()


# ---- mesh scenes: {key: instance_mesh_mb_helpers.desc}, instances [(geomID, key, [local-to-world per step])] --------------------------------
def tri_mesh():
    v, q = iq.bomberman_quads(BOMBERMAN)
    return v, np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.uint32)


def static_scenes():
    v, t = tri_mesh()
    sv, stt = random_soup(50, 7)
    mixed = iq.mixed_scenes(BOMBERMAN)
    return {
        'triangles only': ({'m': imm.desc(tris=(v, t, 0))}, ('m',)),
        'triangles and quads': ({'a': imm.desc(**mixed['a'])}, ('a',)),
        'quads only': ({'m': imm.desc(**iq.quads_only(BOMBERMAN)['m'])}, ('m',)),
        'two triangle scenes, interleaved': ({'p': imm.desc(tris=(v, t, 0)), 'q': imm.desc(tris=(sv, stt, 2))}, ('p', 'q')),
        'two mixed scenes, interleaved': ({k: imm.desc(**s) for k, s in mixed.items()}, ('a', 'b')),
        'triangles beside quads only': ({'p': imm.desc(tris=(sv, stt, 1)), 'q': imm.desc(**iq.quads_only(BOMBERMAN, 4)['m'])}, ('p', 'q', 'q')),
    }


def placed(n, keys, moving):
    """n instances, instance i over keys[i % len(keys)]; moving: steps of 2, 3 and 5 matrices, every third instance static"""
    inst = im.exact_instances(n, keys, moving=True)
    return [(g, k, steps if moving and g % 3 != 1 else steps[:1]) for g, k, steps in inst]


def mesh_cases(label, cfg, scenes, instances, extra=None, modes=(0, 1)):
    for mode in modes:
        dev, top, inner = imm.build(rtc, mode, scenes, instances, cfg, extra)
        digest('%s [%s] mode %d' % (label, cfg, mode), top)
        release(dev, top, inner)


def static_and_instance_mb_cases():
    for name, (scenes, keys) in static_scenes().items():
        for moving in (False, True):
            what = 'kinds 18-21' if moving else 'kinds 14-17'
            inst = placed(5, keys, moving)
            cfgs = ('gpu=none', FULL) if name.startswith('triangles only') and not moving else (FULL,)
            for cfg in cfgs:
                mesh_cases('%s: %s' % (what, name), cfg, scenes, inst)
            # a disabled instance, an instance of an empty scene (left out), a singular transform
            def extra(top, scenes=scenes, keys=keys):
                dev = top.device
                empty = rtc.Scene(dev)
                empty.commit()
                top.add_instance(empty, ih.affine((7, 7, 7)), geom_id=40)
                top._extra_keep = [empty]
                inner0 = top._keep[0]
                top.add_instance(inner0, ih.affine((200, 0, 0)), geom_id=41)
                top.lib.rtcDisableGeometry(top.lib.rtcGetGeometry(top.handle, 41))
                top.add_instance(inner0, ih.affine((-90, 3, 1), (1, 0, 2)), geom_id=42)
            mesh_cases('%s: %s + disabled, empty, singular' % (what, name), FULL, scenes, inst, extra)


def mesh_mb_cases():
    """kinds 22 / 23 and, under mb_bounds=linear,inst_mb_bounds=linear, 30 / 31: scenes (a)-(d), static and moving instances mixed"""
    for name, make, keys in (('a', imm.scenes_a, ('m',)), ('b', imm.scenes_b, ('m',)), ('c', imm.scenes_c, ('m',)), ('d', imm.scenes_d, ('s', 'm'))):
        scenes = make(BOMBERMAN)
        for cfg, what in ((FULL, 'kinds 22-23'), (LIN, 'kinds 30-31')):
            mesh_cases('%s: scene (%s), static instances' % (what, name), cfg, scenes, placed(3, keys, False))
            mesh_cases('%s: scene (%s), static and moving instances' % (what, name), cfg, scenes, placed(7, keys, True))


# the layout cases of tests/test_host_instance_mesh_mb_linear.py (LAYOUTS, _desc, _top): between them 0, 1 and 2 (mod 3) QNode8s in front
# of the QNodeMB8 section
LAYOUTS = {
    'a single instance of a motion-blur tree: no QNode8 at all': ({'a': dict(ntm=60, seed=3)}, 'a', ()),
    'a motion-blur tree whose root is a leaf: no QNodeMB8': ({'a': dict(ntm=3, seed=3)}, 'aa', ()),
    'all four trees in one scene': ({'a': dict(nt=40, ntm=30, nq=24, nqm=20, seed=3)}, 'aaa', (1,)),
    'two scenes, one instanced twice': ({'a': dict(ntm=44, nqm=36, seed=13), 'b': dict(nt=100, ntm=50, seed=23)}, 'aba', ()),
    'a static scene beside a moving one': ({'s': dict(nt=28, nq=32, seed=33), 'm': dict(ntm=70, seed=43)}, 'sm', (0,)),
    'a root-leaf tree beside a full one': ({'a': dict(nt=200, ntm=2, seed=5), 'b': dict(nqm=40, nq=3, seed=7)}, 'abba', (3,)),
}


def random_quads(n, seed):
    rng = np.random.RandomState(seed)
    c = rng.rand(n, 1, 3) * 10.0
    base = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], np.float64)
    v = (c + base + (rng.rand(n, 4, 3) - 0.5) * 0.2).reshape(-1, 3).astype(np.float32)
    return v, np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


def moved(v, nsteps, seed):
    shift = np.random.RandomState(seed).rand(3).astype(np.float32) * 0.5
    return [(v + k * shift).astype(np.float32) for k in range(nsteps)]


def soup_desc(nt=0, ntm=0, nq=0, nqm=0, seed=3):
    out = imm.desc()
    if nt:
        v, t = random_soup(nt, seed)
        out['tris'] = (v, t, 0)
    if ntm:
        v, t = random_soup(ntm, seed + 1)
        out['tris_mb'] = (moved(v, 2, seed + 1), t, 1)
    if nq:
        v, q = random_quads(nq, seed + 2)
        out['quads'] = (v, q, 2)
    if nqm:
        v, q = random_quads(nqm, seed + 3)
        out['quads_mb'] = (moved(v, 3, seed + 3), q, 3)
    return out


def layout_cases():
    for name, (shapes, uses, moving) in LAYOUTS.items():
        scenes = {k: soup_desc(**a) for k, a in shapes.items()}
        inst = []
        for i, k in enumerate(uses):
            m = ih.affine((30.0 * i, 0, 0))
            inst.append((i, k, [m, ih.affine((30.0 * i, 1.0, 0)), ih.affine((30.0 * i, 2.0, 0.5))] if i in moving else [m]))
        for cfg, what in ((LIN, 'kinds 30-31'), (FULL, 'kinds 22-23')):
            mesh_cases('%s layout: %s' % (what, name), cfg, scenes, inst)
    # the key set but no linear accel below: swept motion-blur scenes, and static scenes only
    swept = {'a': soup_desc(40, 30, 24, 20), 'b': soup_desc(24, 0, 0, 0, seed=5)}
    mesh_cases('inst_mb_bounds=linear over swept scenes', FULL + ',inst_mb_bounds=linear', swept, placed(4, ('a', 'b'), True))
    static = {'a': soup_desc(40, 0, 24, 0), 'b': soup_desc(24, 0, 0, 0, seed=5)}
    mesh_cases('linear keys over static scenes', LIN, static, placed(4, ('a', 'b'), False))
    mesh_cases('linear keys over static scenes, moving instances', LIN, static, placed(4, ('a', 'b'), True))


# ---- subdivision scenes (kinds 24 / 25) --------------------------------------------------------------------------------------------------------
def subdiv_case(label, accel, meshes, instances, cfg=SUBDIV, extra=None):
    dev, top, inner = isd.build(rtc, accel, meshes, instances, cfg, extra)
    digest('kinds 24-25: %s [%s,subdiv_accel=%s]' % (label, cfg, accel), top)
    release(dev, top, inner)


def subdiv_cases():
    faces = isd.bomberman_faces(BOMBERMAN)
    moving = isd.lattice_instances(5, keys=('m', 'c'))
    g, k, steps = moving[2]
    moving[2] = (g, k, [steps[0], ih.affine((85.0, 3.0, 1.0), (0.5,) * 3), ih.affine((90.0, -2.0, 4.0), (0.5,) * 3)])
    g, k, steps = moving[3]
    moving[3] = (g, k, [steps[0], ih.affine((125.0, 1.0, -1.0))])
    subdiv_case('eager, one scene', isd.EAGER, {'m': faces + (3, 1)}, isd.lattice_instances(3))
    for c in (1, 2, 3, 4, 5):  # (a scene's commit refuses a compression level above its subdivision level)
        subdiv_case('compressed.leaf C=%d at level %d' % (c, max(2, c)), isd.LEAF, {'m': faces + (max(2, c), c)}, isd.lattice_instances(3))
    for accel in isd.FAMILIES:
        two = {'m': faces + (3, 2), 'c': isd.cube() + (4, 2)}
        subdiv_case('two scenes', accel, two, isd.lattice_instances(5, keys=('m', 'c')))
        subdiv_case('two scenes, moving instances', accel, two, moving)

        def extra(top, dev):
            """geometry of the top scene's own and instances of a mesh scene beside the subdivision instances"""
            v, t = random_soup(20, 3)
            top.add_triangles(v, t, geom_id=20)
            tri = rtc.Scene(dev)
            tri.add_triangles(*random_soup(30, 4))
            tri.add_quads(*random_quads(10, 5))
            tri.commit()
            top.add_instance(tri, ih.affine((-50, 0, 0)), geom_id=21)
            top.add_instance_mb(tri, [ih.affine((-90, 0, 0)), ih.affine((-90, 2, 0))], geom_id=22)
            return [tri]
        subdiv_case('both instance classes beside own geometry', accel, two, moving, SUBDIV + ',quad_accel=default', extra)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def refusal(label, cfg, make):
    """make(dev) -> (top scene, scenes to release); the top scene's commit is expected to fail"""
    dev = rtc.Device(cfg)
    log = []
    fn = ERRFN(lambda user, code, msg: log.append((code, (msg or b'').decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(fn, C.c_void_p), None)
    top, keep = make(dev)
    del log[:]
    top.lib.rtcCommitScene(top.handle)
    code = dev.error()
    print('refusal: %s [%s] | code %d | %s' % (label, cfg, code, ' || '.join('%d: %s' % e for e in log)), flush=True)
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, None, None)
    top.release()
    for s in keep:
        s.release()
    dev.release()


def scene_of(dev, flags=0, tris=None, quads=None, tris_mb=None, quads_mb=None, commit=True):
    sc = rtc.Scene(dev, flags)
    if tris:
        sc.add_triangles(*random_soup(tris, 1))
    if quads:
        sc.add_quads(*random_quads(quads, 2))
    if tris_mb:
        v, t = random_soup(tris_mb, 3)
        sc.add_triangles_mb(moved(v, 2, 3), t)
    if quads_mb:
        v, q = random_quads(quads_mb, 4)
        sc.add_quads_mb(moved(v, 2, 4), q)
    if commit:
        sc.commit()
    return sc


def over(dev, inner, flags=0, xfms=None):
    """a top scene with one instance per entry of `inner`, geomIDs 3, 5, 7, ..."""
    top = rtc.Scene(dev, flags)
    for i, s in enumerate(inner):
        top.add_instance(s, ih.affine((20.0 * i, 0, 0)) if xfms is None else xfms[i], geom_id=3 + 2 * i)
    return top, list(inner)


def subdiv_inner(dev, L=2, Cl=1, filt=None, beside=None):
    sc = rtc.Scene(dev)
    gid = sc.add_subdiv(*isd.cube())
    sc.set_levels(L, Cl)
    if filt is not None:
        g = dev.lib.rtcGetGeometry(sc.handle, gid)
        dev.lib.rtcSetGeometryIntersectFilterFunction(g, C.cast(filt, C.c_void_p))
        dev.lib.rtcCommitGeometry(g)
    if beside is not None:
        beside(sc)
    sc.commit()
    return sc


def refusals():
    R, QV = rtc.RTC_SCENE_FLAG_ROBUST, 'gpu=none,quad_accel=bvh8.quad4v,inst_accel=default'
    keep_fn = rtc.FILTER_FUNC(lambda args: None)

    def with_filter(dev, **parts):
        sc = scene_of(dev, commit=False, **parts)
        sc.set_filters(0, intersect=keep_fn)
        sc.commit()
        return sc

    def no_scene(dev):
        top = rtc.Scene(dev)
        g = dev.lib.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_INSTANCE)
        dev.lib.rtcCommitGeometry(g)
        dev.lib.rtcAttachGeometry(top.handle, g)
        dev.lib.rtcReleaseGeometry(g)
        return top, []

    def nested(dev, **parts):
        leaf = scene_of(dev, **parts)
        mid, _ = over(dev, [leaf])
        mid.commit()
        top, _ = over(dev, [mid])
        return top, [mid, leaf]

    def moving_instance(dev):
        inner = scene_of(dev, tris=8)
        top = rtc.Scene(dev)
        top.add_instance_mb(inner, [ih.affine(), ih.affine((1, 0, 0))], geom_id=2)
        return top, [inner]

    def not_finite(dev):
        inner = scene_of(dev, tris=8)
        top = rtc.Scene(dev)
        top.add_instance(inner, geom_id=0)
        top.add_instance_mb(inner, [ih.affine(), ih.affine((3e38, 0, 0), (3e38, 1, 1))], geom_id=1)
        return top, [inner]

    # the mesh builder, in the order of its checks
    refusal('unknown inst_accel (any scene)', 'gpu=none,inst_accel=bvh4.object', lambda dev: (scene_of(dev, tris=8, commit=False), []))
    refusal('instance with time steps, plain host-only device', 'gpu=none', moving_instance)
    refusal('instance without a scene', FULL, no_scene)
    refusal('uncommitted instanced scene', FULL, lambda dev: over(dev, [scene_of(dev, tris=8, commit=False)]))
    refusal('uncommitted scene behind a committed one', FULL, lambda dev: over(dev, [scene_of(dev, tris=8), scene_of(dev, tris=8, commit=False)]))
    for cfg in (FULL + ',mb_bounds=linear', FULL + ',mb_bounds=linear,inst_mb_bounds=swept'):
        refusal('linear accel below, key not set', cfg, lambda dev: over(dev, [scene_of(dev, tris=8, tris_mb=20)]))
        refusal('linear quad accel below, key not set', cfg, lambda dev: over(dev, [scene_of(dev, quads_mb=20)]))
    refusal('quads below, triangles-only device', 'gpu=none,quad_accel=default', lambda dev: over(dev, [scene_of(dev, tris=8, quads=8)]))
    refusal('time steps below, triangles-only device', 'gpu=none', lambda dev: over(dev, [scene_of(dev, tris_mb=8)]))
    refusal('time steps below, static device', 'gpu=none,quad_accel=default,inst_accel=default', lambda dev: over(dev, [scene_of(dev, tris=8, tris_mb=8)]))
    refusal('subdivision below, triangles-only device', 'gpu=none', lambda dev: over(dev, [subdiv_inner(dev)]))
    refusal('subdivision below, static device', 'gpu=none,inst_accel=default', lambda dev: over(dev, [subdiv_inner(dev)]))
    refusal('subdivision below, mesh motion device', FULL, lambda dev: over(dev, [subdiv_inner(dev)]))
    refusal('instance below an instance, triangles-only device', 'gpu=none', lambda dev: nested(dev, tris=8))
    refusal('instance below an instance, static device', 'gpu=none,inst_accel=default', lambda dev: nested(dev, tris=8))
    refusal('instance below an instance, mesh motion device', FULL, lambda dev: nested(dev, tris=8, tris_mb=8))
    refusal('instance below an instance, subdivision device', SUBDIV + ',subdiv_accel=default', lambda dev: nested(dev, tris=8))
    refusal('geometry filter below', FULL, lambda dev: over(dev, [with_filter(dev, tris=8)]))
    refusal('geometry filter on a moving mesh below', FULL, lambda dev: over(dev, [with_filter(dev, tris_mb=8)]))
    refusal('accels of one scene disagree, motion blur involved', FULL + ',tri_accel_mb=bvh8.triangle4imb',
            lambda dev: over(dev, [scene_of(dev, R, tris=8, tris_mb=8)], R))
    refusal('scenes disagree, motion blur involved (first check)', FULL,
            lambda dev: over(dev, [scene_of(dev, R, tris=8), scene_of(dev, 0, tris_mb=8, quads=4)], R))
    refusal('scenes disagree, motion blur in the first scene', FULL,
            lambda dev: over(dev, [scene_of(dev, 0, tris_mb=8, quads_mb=4), scene_of(dev, R, tris=8, quads=4)]))
    refusal('triangle and quad accels of one scene disagree', QV, lambda dev: over(dev, [scene_of(dev, R, tris=8, quads=8)], R))
    refusal('triangle scenes disagree', 'gpu=none', lambda dev: over(dev, [scene_of(dev, R, tris=8), scene_of(dev, 0, tris=8)], R))
    refusal('scenes disagree, quads involved', FULL, lambda dev: over(dev, [scene_of(dev, R, tris=8, quads=8), scene_of(dev, 0, tris=8)], R))
    refusal('scenes disagree, quads in the second scene', FULL, lambda dev: over(dev, [scene_of(dev, R, tris=8), scene_of(dev, 0, quads=8)], R))
    refusal('bounds not finite', FULL, lambda dev: over(dev, [scene_of(dev, tris=8)], xfms=[ih.affine((3e38, 0, 0), (3e38, 1, 1))]))
    refusal('bounds of a step not finite', FULL, not_finite)
    # where several apply: the first instance in geomID order decides, and within it the order of the checks
    refusal('second instance refused before the first one\'s bounds', FULL,
            lambda dev: over(dev, [scene_of(dev, tris=8), with_filter(dev, tris=8)], xfms=[ih.affine(), ih.affine((3e38, 0, 0), (3e38, 1, 1))]))
    refusal('not finite bounds of the first instance before the second one\'s filter', FULL,
            lambda dev: over(dev, [scene_of(dev, tris=8), with_filter(dev, tris=8)], xfms=[ih.affine((3e38, 0, 0), (3e38, 1, 1)), ih.affine()]))
    refusal('mesh refusal before the subdivision builder\'s', SUBDIV + ',subdiv_accel=bvh4.compressed.box',
            lambda dev: over(dev, [subdiv_inner(dev), with_filter(dev, tris=8)]))

    # the subdivision builder
    tri = lambda sc: sc.add_triangles(*random_soup(8, 1))  # noqa: E731
    quad = lambda sc: sc.add_quads(*random_quads(2, 1))  # noqa: E731
    SD = SUBDIV + ',quad_accel=default,subdiv_accel='

    def beside_instance(dev):
        leaf = scene_of(dev, tris=8)
        inner = subdiv_inner(dev, beside=lambda sc: sc.add_instance(leaf))
        top, keep = over(dev, [inner])
        return top, keep + [leaf]

    refusal('subdivision beside an instance', SD + 'default', beside_instance)
    refusal('subdivision beside triangles', SD + 'default', lambda dev: over(dev, [subdiv_inner(dev, beside=tri)]))
    refusal('subdivision beside quads', SD + 'default', lambda dev: over(dev, [subdiv_inner(dev, beside=quad)]))
    refusal('filter on subdivision geometry below', SD + 'default', lambda dev: over(dev, [subdiv_inner(dev, filt=keep_fn)]))
    for mode in ('box', 'grid', 'full'):
        refusal('compressed.%s below an instance' % mode, SD + 'bvh4.compressed.' + mode, lambda dev: over(dev, [subdiv_inner(dev)]))
    refusal('compression levels disagree', SD + 'bvh4.compressed.leaf', lambda dev: over(dev, [subdiv_inner(dev, 3, 2), subdiv_inner(dev, 3, 3)]))
    refusal('not finite bounds of a subdivision instance', SD + 'default', lambda dev: over(dev, [subdiv_inner(dev)], xfms=[ih.affine((3e38, 0, 0), (3e38, 1, 1))]))
    refusal('subdivision instances: the first in geomID order decides', SD + 'default',
            lambda dev: over(dev, [subdiv_inner(dev, beside=quad), subdiv_inner(dev, filt=keep_fn)]))


# ---- the primitive builders: triangles, quads, curves, lines; static and with time steps ------------------------------------------------------
PRIM_KEYS = dict(quad_accel='default', quad_accel_mb='default', tri_accel_mb='default', line_accel_mb='default', hair_accel='default')
# type -> (device key, the names its builder accepts, moving)
PRIM_TYPES = {
    'tri': ('tri_accel', ('default', 'bvh8.triangle4v', 'bvh4.triangle4v', 'bvh8.triangle4', 'bvh4.triangle4', 'qbvh8.triangle4'), False),
    'trimb': ('tri_accel_mb', ('default', 'bvh8.triangle4imb', 'bvh4.triangle4imb', 'bvh8.triangle4vmb', 'bvh4.triangle4vmb'), True),
    'quad': ('quad_accel', ('default', 'bvh8.quad4v', 'bvh4.quad4v', 'bvh8.quad4i', 'bvh4.quad4i', 'qbvh8.quad4i'), False),
    'quadmb': ('quad_accel_mb', ('default', 'bvh8.quad4imb', 'bvh4.quad4imb'), True),
    'curve': ('hair_accel', ('default', 'bvh4.bezier1v', 'bvh4.bezier1i', 'bvh4obb.bezier1v', 'bvh4obb.bezier1i', 'bvh8obb.bezier1v', 'bvh8obb.bezier1i'), False),
    'line': ('line_accel', ('default', 'bvh8.line4i', 'bvh4.line4i'), False),
    'linemb': ('line_accel_mb', ('default', 'bvh8.line4imb', 'bvh4.line4imb'), True),
}
SIZES = (1, 4, 5, 29, 300)  # the root is a leaf; a full block; one over it; one over the largest leaf; several levels
FLAGS = (rtc.RTC_SCENE_FLAG_NONE, rtc.RTC_SCENE_FLAG_ROBUST)


def prim_cfg(*extra, **keys):
    """a host-only device config that names every key a host-only device needs, `keys` replacing the defaults"""
    k = dict(PRIM_KEYS, **keys)
    return ','.join(['gpu=none'] + ['%s=%s' % kv for kv in k.items()] + list(extra))


def prim_gen(typ, n, seed, steps=2):
    """(vertices, index) of n primitives of a type; vertices of a moving type: one array per time step (the radius moves too)"""
    rng = np.random.RandomState(1000 + seed)
    base = typ.replace('mb', '')
    if base == 'tri':
        v, idx = random_soup(n, seed)
    elif base == 'quad':
        v, idx = random_quads(n, seed)
    else:
        k = 2 if base == 'line' else 4
        c = rng.rand(n, 1, 3) * 10.0
        v = np.concatenate([c + (rng.rand(n, k, 3) - 0.5), 0.01 + 0.2 * rng.rand(n, k, 1)], 2).reshape(-1, 4).astype(np.float32)
        idx = np.arange(0, k * n, k, dtype=np.uint32)
    if not PRIM_TYPES[typ][2]:
        return v, idx
    shift = np.zeros(v.shape[1], np.float32)
    shift[:3] = rng.rand(3) * 0.5
    if v.shape[1] == 4:
        shift[3] = 0.03
    return [(v + s * shift * (1.0 + 0.25 * s)).astype(np.float32) for s in range(steps)], idx


def prim_put(sc, typ, v, idx, geom_id=None, **kw):
    add = {'tri': sc.add_triangles, 'trimb': sc.add_triangles_mb, 'quad': sc.add_quads, 'quadmb': sc.add_quads_mb, 'curve': sc.add_curves, 'line': sc.add_lines,
           'linemb': sc.add_lines_mb}[typ]
    return add(v, idx, geom_id=geom_id, **kw)


def prim_scene(label, cfg, parts, flags=0, after=None):
    """parts: [(type, vertices, index, keywords of the add call)]; after(scene): further set-up in front of the commit"""
    dev = rtc.Device(cfg)
    sc = rtc.Scene(dev, flags)
    for typ, v, idx, kw in parts:
        prim_put(sc, typ, v, idx, **kw)
    if after:
        after(sc)
    sc.commit()
    digest('%s [%s] flags %d' % (label, cfg, flags), sc)
    return dev, sc


def prim_case(label, cfg, parts, flags=0, after=None):
    dev, sc = prim_scene(label, cfg, parts, flags, after)
    sc.release()
    dev.release()


def bounds_modes(typ):
    return ((), ('mb_bounds=linear',)) if PRIM_TYPES[typ][2] else ((),)


def prim_size_cases():
    for typ, (key, names, moving) in PRIM_TYPES.items():
        for name in names:
            for extra in bounds_modes(typ):
                for n in SIZES:
                    for flags in FLAGS:
                        v, idx = prim_gen(typ, n, n, steps=3 if n == 29 else 2)
                        prim_case('%s: %d primitives' % (typ, n), prim_cfg(*extra, **{key: name}), [(typ, v, idx, {})], flags)


def prim_skipped_cases():
    """12 primitives: 1 has a NaN coordinate, 3 the first index that reaches past the vertex buffer, 4 an index far outside, 5 a value above
    FLT_LARGE, 7 (lines, curves) a negative radius, and with time steps 9 is invalid at the middle step 1 of four only"""
    for typ, (key, names, moving) in PRIM_TYPES.items():
        v, idx = prim_gen(typ, 12, 77, steps=4)
        idx = idx.copy()
        steps = v if moving else [v]
        per = len(steps[0]) // 12  # vertices per primitive
        nv = len(steps[0])
        for s, a in enumerate(steps):
            a[1 * per, 1] = np.nan
            a[5 * per + per - 1, 2] = 1.0e19
            if a.shape[1] == 4:
                a[7 * per, 3] = -0.01
            if moving and s == 1:
                a[9 * per, 0] = np.inf
        if idx.ndim == 2:
            idx[3, 1] = nv
            idx[4, 2] = nv + 1000
        else:
            idx[3] = nv - per + 1
            idx[4] = nv + 1000
        for extra in bounds_modes(typ):
            for flags in FLAGS:
                prim_case('%s: skipped primitives' % typ, prim_cfg(*extra), [(typ, v, idx, {})], flags)


def prim_shape_cases():
    for typ, (key, names, moving) in PRIM_TYPES.items():
        static = typ.replace('mb', '') if typ != 'curve' else 'curve'
        for extra in bounds_modes(typ):
            def some(n, seed, gid, steps=2, t=typ):
                v, idx = prim_gen(t, n, seed, steps)
                return (t, v, idx, dict(geom_id=gid))
            ev, eidx = prim_gen(typ, 3, 5)
            empty = (typ, ev, eidx[:0], dict(geom_id=6))
            # gaps in the IDs, a disabled geometry (ID 2), a geometry without primitives (ID 6)
            prim_case('%s: gaps, disabled, empty' % typ, prim_cfg(*extra), [some(9, 1, 1), some(7, 2, 2), some(40, 3, 4), empty, some(5, 4, 9)],
                      after=lambda sc: sc.set_enabled(2, False))
            prim_case('%s: nothing but a disabled and an empty geometry' % typ, prim_cfg(*extra), [some(7, 2, 2), empty], after=lambda sc: sc.set_enabled(2, False))
            if moving:
                # time-step counts 2, 3 and 5 under interleaved IDs, alone and with static geometries of the type in between
                mixed = [some(11, 1, 0, 2), some(13, 2, 2, 3), some(17, 3, 5, 5)]
                prim_case('%s: time steps 2, 3, 5' % typ, prim_cfg(*extra), mixed)
                prim_case('%s: time steps 2, 3, 5 between static geometries' % typ, prim_cfg(*extra), mixed + [some(6, 4, 1, t=static), some(8, 5, 3, t=static)])
    # Bezier beside B-spline, tessellation rates 1, 4, 16 and NaN (and what the clamp makes of others)
    rates = (1, 4, 16, float('nan'), 0.5, 7.9, 100, None)
    both = []
    for i, rate in enumerate(rates):
        for j, basis in enumerate(('bezier', 'bspline')):
            v, idx = prim_gen('curve', 9 + i, 10 * i + j)
            kw = dict(basis=basis, tessellation_rate=rate)
            prim_case('curve: %s, tessellation rate %s' % (basis, rate), prim_cfg(), [('curve', v, idx, kw)])
            both.append(('curve', v, idx, dict(kw, geom_id=3 * len(both) + 1)))
    for flags in FLAGS:
        prim_case('curve: Bezier beside B-spline, all rates', prim_cfg(), both, flags)


def prim_exported_cases():
    """what the inspection calls describe: every pair of the seven types, and all of them"""
    types = list(PRIM_TYPES)
    part = {t: (t,) + prim_gen(t, 6 + i, 20 + i) + ({},) for i, t in enumerate(types)}
    for i, a in enumerate(types):
        for b in types[i + 1:]:
            prim_case('exported: %s + %s' % (a, b), prim_cfg(), [part[b], part[a]])
    for extra in ((), ('mb_bounds=linear',)):
        prim_case('exported: all seven types', prim_cfg(*extra), [part[t] for t in reversed(types)])


def prim_recommit_cases():
    """commit; disable the type's geometry (its accel becomes empty), commit; enable it and move a vertex, commit: alone in the scene and beside
    a geometry of the type behind it in the order of the inspection calls"""
    types = list(PRIM_TYPES)
    for i, typ in enumerate(types):
        for other in (None, types[(i + 1) % len(types)]):
            v, idx = prim_gen(typ, 33, 40 + i, steps=3)
            parts = [(typ, v, idx, dict(geom_id=0))]
            if other:
                parts.append((other,) + prim_gen(other, 10, 50 + i) + (dict(geom_id=1),))
            label = 'recommit: %s%s' % (typ, ' beside ' + other if other else '')
            dev, sc = prim_scene(label + ', first commit', prim_cfg(), parts)
            sc.set_enabled(0, False)
            sc.commit()
            digest(label + ', disabled', sc)
            sc._keep[0][0, :3] += 25.0  # the first vertex of geometry 0 (at its first time step), in the shared buffer the geometry reads in place
            sc.set_enabled(0, True)
            sc.commit()
            digest(label + ', enabled and changed', sc)
            sc.release()
            dev.release()


def raw_geometry(sc, gtype, steps, vertex, index, bound_steps=None, fmt=None):
    """a geometry with `steps` time steps of which only the first `bound_steps` get a vertex buffer (the wrappers of rtc.py always bind all)"""
    L, dev = sc.lib, sc.device
    g = L.rtcNewGeometry(dev.handle, gtype)
    dev.check('rtcNewGeometry')
    L.rtcSetGeometryTimeStepCount(g, steps)
    wide = vertex.shape[1] == 4
    for slot in range(steps if bound_steps is None else bound_steps):
        vpad = np.zeros((vertex.shape[0] + 2, vertex.shape[1]), np.float32)
        vpad[:vertex.shape[0]] = vertex + np.float32(0.25 * slot)
        L.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, slot, rtc.RTC_FORMAT_FLOAT4 if wide else rtc.RTC_FORMAT_FLOAT3, vpad.ctypes.data, 0, 4 * vertex.shape[1],
                                     vertex.shape[0])
        sc._keep.append(vpad)
    idx = np.ascontiguousarray(index, np.uint32)
    L.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_INDEX, 0, fmt, idx.ctypes.data, 0, idx.itemsize * (idx.shape[1] if idx.ndim == 2 else 1), idx.shape[0])
    sc._keep.append(idx)
    L.rtcCommitGeometry(g)
    L.rtcAttachGeometry(sc.handle, g)
    L.rtcReleaseGeometry(g)
    dev.check('raw_geometry')


def prim_refusals():
    def scene(*types, raw=()):
        def make(dev):
            sc = rtc.Scene(dev)
            for i, t in enumerate(types):
                prim_put(sc, t, *prim_gen(t, 6, 60 + i))
            for r in raw:
                r(sc)
            return sc, []
        return make

    def curves_with_steps(sc):
        v, idx = prim_gen('curve', 5, 70)
        raw_geometry(sc, rtc.RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE, 2, v, idx, fmt=rtc.RTC_FORMAT_UINT)

    def step_without_buffer(typ):
        gtype, fmt = {'trimb': (rtc.RTC_GEOMETRY_TYPE_TRIANGLE, rtc.RTC_FORMAT_UINT3), 'quadmb': (rtc.RTC_GEOMETRY_TYPE_QUAD, rtc.RTC_FORMAT_UINT4),
                      'linemb': (rtc.RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE, rtc.RTC_FORMAT_UINT)}[typ]
        v, idx = prim_gen(typ.replace('mb', ''), 5, 71)
        return lambda sc: raw_geometry(sc, gtype, 3, v, idx, bound_steps=2, fmt=fmt)

    bad = 'bvh7.nonsense'
    for typ, (key, names, moving) in PRIM_TYPES.items():
        refusal('unknown %s' % key, prim_cfg(**{key: bad}), scene(typ))
        refusal('unknown %s, no geometry of the type' % key, prim_cfg(**{key: bad}), scene('tri' if typ != 'tri' else 'quad'))
    # time steps on a device that lacks the key
    refusal('quads with time steps, no quad_accel_mb', 'gpu=none,quad_accel=default', scene('quadmb'))
    refusal('lines with time steps, no line_accel_mb', 'gpu=none', scene('linemb'))
    refusal('lines with time steps beside static lines, no line_accel_mb', 'gpu=none,hair_accel=default', scene('line', 'linemb'))
    refusal('curves with time steps', prim_cfg(), scene('curve', raw=[curves_with_steps]))
    for typ in ('trimb', 'quadmb', 'linemb'):
        for extra in bounds_modes(typ):
            refusal('%s: a time step without a vertex buffer' % typ, prim_cfg(*extra), scene(typ, raw=[step_without_buffer(typ)]))
    # two faults in one scene: the builder that runs first reports (triangles, motion-blur triangles, quads, motion-blur quads, subdivision,
    # curves, lines, motion-blur lines)
    refusal('unknown tri_accel and unknown line_accel', prim_cfg(tri_accel=bad, line_accel=bad + '2'), scene('line', 'tri'))
    refusal('unknown line_accel_mb and unknown tri_accel_mb', prim_cfg(line_accel_mb=bad, tri_accel_mb=bad + '2'), scene('linemb', 'trimb'))
    refusal('quad time steps and unknown hair_accel', 'gpu=none,quad_accel=default,hair_accel=' + bad, scene('curve', 'quadmb'))
    refusal('unknown quad_accel and line time steps', 'gpu=none,quad_accel=' + bad, scene('linemb', 'quad'))
    refusal('unknown hair_accel and line time steps', 'gpu=none,hair_accel=' + bad, scene('linemb', 'curve'))
    refusal('curve time steps and unknown line_accel', prim_cfg(line_accel=bad), scene('line', raw=[curves_with_steps]))
    refusal('line time steps and unknown quad_accel_mb', 'gpu=none,quad_accel_mb=' + bad, scene('quad', 'linemb'))
    refusal('a time step without a vertex buffer (triangles) and unknown quad_accel', prim_cfg(quad_accel=bad), scene('quad', raw=[step_without_buffer('trimb')]))
    refusal('unknown tri_accel_mb and a time step without a vertex buffer (lines)', prim_cfg(tri_accel_mb=bad), scene('tri', raw=[step_without_buffer('linemb')]))


def prim_verbose_child(typ, linear):
    prim_case('verbose', prim_cfg('verbose=2', *(['mb_bounds=linear'] if linear else [])), [(typ,) + prim_gen(typ, 50, 9) + ({},)])


def prim_cases():
    prim_size_cases()
    prim_skipped_cases()
    prim_shape_cases()
    prim_exported_cases()
    prim_recommit_cases()
    prim_refusals()


# ---- the verbose=2 lines ------------------------------------------------------------------------------------------------------------------------
def verbose_child(kind):
    if kind.split('+')[0] in PRIM_TYPES:
        return prim_verbose_child(kind.split('+')[0], kind.endswith('+linear'))
    kind = int(kind)
    if kind == 25:
        dev, top, inner = isd.build(rtc, isd.LEAF, {'c': isd.cube() + (3, 2)}, placed(4, ('c',), True), SUBDIV + ',verbose=2')
    elif kind == 21:  # (below the kinds 22 / 23 the line's "instanced quads" counts the InstanceSteps too)
        dev, top, inner = imm.build(rtc, 1, {k: imm.desc(**s) for k, s in iq.mixed_scenes(BOMBERMAN).items()}, placed(5, ('a', 'b'), True), FULL + ',verbose=2')
    else:
        dev, top, inner = imm.build(rtc, 1, imm.scenes_c(BOMBERMAN), placed(7, ('m',), True), (LIN if kind == 31 else FULL) + ',verbose=2')
    assert top.stats()['accelKind'] == kind
    release(dev, top, inner)


def verbose_lines():
    for kind in list(PRIM_TYPES) + [t + '+linear' for t in PRIM_TYPES if PRIM_TYPES[t][2]] + [21, 23, 25, 31]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--verbose-child', str(kind)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
        for line in r.stderr.splitlines():
            print('verbose=2, %s | %s' % ('kind %d' % kind if isinstance(kind, int) else kind, line), flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--verbose-child':
        verbose_child(sys.argv[2])
        sys.exit(0)
    prim_cases()
    static_and_instance_mb_cases()
    mesh_mb_cases()
    layout_cases()
    subdiv_cases()
    refusals()
    verbose_lines()
