"""Development check, CPU only: digest of what the two instance builders (csrc/rt_instance_build.cpp) make of a fixed list of host-only
scenes.  One line per case: accel kind, root, every field of rtcamdGetSceneStats, rtcGetSceneBounds, and a SHA-256 per exported array
(rtcamdGetAccelData 0..3 and 16..19); one line per refusal: error code and the full message; and the verbose=2 lines of one scene each of
the kinds 21, 23, 25 and 31 (printed by a child process, which this tool starts).  Run it once per library build (RTAMD_LIB=...) and
`diff` the listings: no difference = byte-identical accels, the same refusals.  The scenes come from the helper modules of tests/.
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


# ---- the verbose=2 lines ------------------------------------------------------------------------------------------------------------------------
def verbose_child(kind):
    if kind == 25:
        dev, top, inner = isd.build(rtc, isd.LEAF, {'c': isd.cube() + (3, 2)}, placed(4, ('c',), True), SUBDIV + ',verbose=2')
    elif kind == 21:  # (below the kinds 22 / 23 the line's "instanced quads" counts the InstanceSteps too)
        dev, top, inner = imm.build(rtc, 1, {k: imm.desc(**s) for k, s in iq.mixed_scenes(BOMBERMAN).items()}, placed(5, ('a', 'b'), True), FULL + ',verbose=2')
    else:
        dev, top, inner = imm.build(rtc, 1, imm.scenes_c(BOMBERMAN), placed(7, ('m',), True), (LIN if kind == 31 else FULL) + ',verbose=2')
    assert top.stats()['accelKind'] == kind
    release(dev, top, inner)


def verbose_lines():
    for kind in (21, 23, 25, 31):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--verbose-child', str(kind)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
        for line in r.stderr.splitlines():
            print('verbose=2, kind %d | %s' % (kind, line), flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--verbose-child':
        verbose_child(int(sys.argv[2]))
        sys.exit(0)
    static_and_instance_mb_cases()
    mesh_mb_cases()
    layout_cases()
    subdiv_cases()
    refusals()
    verbose_lines()
