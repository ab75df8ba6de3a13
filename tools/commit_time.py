"""Development measurement, CPU only: wall time of Scene.commit() on a host-only device for four large scenes - a soup of 1 M triangles,
1 M static line segments, 250 k Bezier curves, 500 k two-step moving triangles under mb_bounds=linear - for two builds of the library in
turn (A, B, A, B, ...), every run in a process of its own.  Prints one line per run and, per scene and library, mean, minimum and maximum.
usage: commit_time.py LIB_A LIB_B [pairs]          (commit_time.py --run SCENE is the child)"""
import importlib
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
CFG = 'gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,line_accel_mb=default,hair_accel=default'
SCENES = ('triangles 1M', 'lines 1M', 'curves 250k', 'moving triangles 500k linear')


def run(scene):
    sys.path.insert(0, ROOT)
    import numpy as np
    rtc = importlib.import_module('embree-compressed_amd').rtc
    rng = np.random.RandomState(5)
    dev = rtc.Device(CFG + (',mb_bounds=linear' if 'linear' in scene else ''))
    sc = rtc.Scene(dev)

    def points(n, k, width):  # n primitives of k points each, spread over [0, 100]^3
        c = rng.rand(n, 1, 3) * 100.0
        p = c + (rng.rand(n, k, 3) - 0.5)
        if width == 4:
            p = np.concatenate([p, 0.01 + 0.05 * rng.rand(n, k, 1)], 2)
        return p.reshape(-1, width).astype(np.float32)

    if scene == SCENES[0]:
        sc.add_triangles(points(1000000, 3, 3), np.arange(3000000, dtype=np.uint32).reshape(-1, 3))
    elif scene == SCENES[1]:
        sc.add_lines(points(1000000, 2, 4), np.arange(0, 2000000, 2, dtype=np.uint32))
    elif scene == SCENES[2]:
        sc.add_curves(points(250000, 4, 4), np.arange(0, 1000000, 4, dtype=np.uint32))
    else:
        v = points(500000, 3, 3)
        sc.add_triangles_mb([v, v + np.float32(0.25)], np.arange(1500000, dtype=np.uint32).reshape(-1, 3))
    t0 = time.perf_counter()
    sc.commit()
    print('%.4f' % (time.perf_counter() - t0))
    sc.release()
    dev.release()


if __name__ == '__main__':
    if sys.argv[1] == '--run':
        run(sys.argv[2])
        sys.exit(0)
    libs, pairs = sys.argv[1:3], int(sys.argv[3]) if len(sys.argv) > 3 else 5
    for scene in SCENES:
        times = {lib: [] for lib in libs}
        for k in range(pairs):
            for lib in libs:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--run', scene], env=dict(os.environ, RTAMD_LIB=lib), stdout=subprocess.PIPE, text=True, check=True)
                times[lib].append(float(out.stdout.split()[-1]))
                print('%s | %s | run %d | %.4f s' % (scene, lib, k, times[lib][-1]), flush=True)
        for lib in libs:
            t = times[lib]
            print('%s | %s | mean %.4f s, min %.4f, max %.4f' % (scene, lib, sum(t) / len(t), min(t), max(t)), flush=True)
