"""A float64 ground truth for the cBVH encoder and the subdivision kernels, in plain numpy (tests/test_host_cbvh_encoder_truth.py,
tests/test_host_cbvh_ray_truth.py, tests/test_gpu_cbvh_truth.py).

Everything the suite expects of a cBVH blob so far came out of the product's own encoder.  Here a blob is derived a second time, from the kept vertex grid
alone (keep_grids=1, accel_data(4)), after the description of the algorithm in DESIGN.md section 5 / 6 and the comments of csrc/cbvh_encode.cpp: whole
arrays at a time, float64 throughout, numpy.linalg.solve for the homographies.  And the surface itself - the two triangles of every cell of the kept
grids - is traced by brute force in float64, which knows nothing of frames, node words or blobs.

  fallback_mesh()        a second, procedural mesh whose patches defeat the perspective frame
  ref_blob()             the float64 derivation of one blob
  plane_positions() ...  the pieces of it that the tests also apply to boxes decoded from the product's words
  brute_force()          closest hit of every ray over all triangles of the kept grids"""
import numpy as np

T_BORDER = np.array([0.0, 0.005, 0.01, 0.05, 0.1, 0.2, 0.4, 0.6], np.float32).astype(np.float64)
T_MID = np.array([0.0, 0.4, 0.48, 0.49, 0.5, 0.51, 0.52, 0.6], np.float32).astype(np.float64)
T_Z = np.array([0.0, 0.25, 0.5, 0.75], np.float32).astype(np.float64)
# the ten planes of a node word in the order of plane_positions(): (table, bit offset in the 32-bit word, number of bits)
PLANES = (("X1", T_BORDER, 5, 3), ("X2", T_MID, 2, 3), ("X3", T_MID, 13, 3), ("X4", T_BORDER, 10, 3),
          ("Y1", T_BORDER, 21, 3), ("Y2", T_MID, 18, 3), ("Y3", T_MID, 29, 3), ("Y4", T_BORDER, 26, 3),
          ("minZ", T_Z, 0, 2), ("maxZ", T_Z, 16, 2))
MAX_EXTENT = 1.0
TIE = 1e-6  # a float64 inequality closer to a tie than this (relative to the blob's coordinates) is not held against the fp32 encoder


# ---------------------------------------------------------------------------------------------------------------- meshes
def fallback_mesh(stretch=-1.5):
    """(verts float32 [n,3], face sizes, face indices): a sheet of 5 x 6 quads (30 faces, 42 vertices on the 2^-10 grid), rows along y.

    The perspective modes accept a blob only if, in the frame spanned by its corner vertices, x never decreases along a grid row and y never along a
    grid column ("proper alignment"); otherwise the blob falls back to the affine map of its local bounding box.  Two regions:
      rows 0..3 of the control cage: an axis-aligned lattice (x_i, y_j, 1/2) with uneven spacing.  The limit surface over the 16 control points of an interior face is then the
                plane z = 1/2 itself, on an axis-aligned frame: blobs whose z range is exactly 0 (the encoder's flat path), and well-aligned ones;
      rows 4..6: row 4 and row 6 are mirrored about the sheet's centre line and stretched by 1.5, row 5 is not.  The u direction of the limit surface
                turns round between two such rows, so the bands of faces between rows 3 .. 6 hold the line where it vanishes: a blob that holds the
                line has rows that run forwards and rows that run backwards in any frame.  Heights there are scattered by multiples of 1/8, so that no
                blob's frame is degenerate by symmetry.  The surface passes through itself, which a ray tracer does not mind.
    Measured with alignment_margin() in float64 (the host test asserts >= 25 % of the blobs in the fallback, >= 25 % not, >= 1 flat, per perspective
    mode): 40 % of the 120 blobs at (L, C) = (2, 1), 63 % of the 30 blobs at (3, 3) and (5, 5); 40 / 10 / 10 flat blobs."""
    nx, ny = 6, 7
    mirror = {4: stretch, 6: stretch}
    xs, ys = (0.0, 1.0, 2.125, 3.0, 4.25, 5.0), (0.0, 1.125, 2.0, 3.25, 4.0, 5.0, 6.0)  # uneven: on an even lattice every mid plane sits exactly on the table's 0.5
    v = []
    for j in range(ny):
        for i in range(nx):
            x, y, z = xs[i], ys[j], 0.5
            if j >= 4:
                x = 2.5 + mirror.get(j, 1.0) * (xs[i] - 2.5)
                z = 0.5 + 0.125 * (((i * 7 + j * 3) % 5) - 2)
            v.append((x, y, z))
    v = np.round(np.array(v) * 1024.0) / 1024.0
    faces = [(r * nx + c, r * nx + c + 1, (r + 1) * nx + c + 1, (r + 1) * nx + c) for r in range(ny - 1) for c in range(nx - 1)]
    return v.astype(np.float32), np.full(len(faces), 4, np.uint32), np.array(faces, np.uint32).ravel()


def kept_grids(sc, L):
    """{primID: float32 [3, w, w]} of a scene committed on a keep_grids=1 device, w = 2^L + 1; [k, row (v direction), column (u direction)]"""
    raw = sc.accel_data(4)
    w = 2 ** L + 1
    per = 12 + 12 * w * w
    out = {}
    for p in range(len(raw) // per):
        h = raw[p * per: p * per + 12].view(np.uint32)
        out[int(h[1])] = raw[p * per + 12: (p + 1) * per].view(np.float32).reshape(3, w, w)
    return out


def window(grid, x0, y0, C):
    """the (2^C+1)^2 vertices of one blob as float64 [row, column, xyz]"""
    s = 2 ** C + 1
    return np.moveaxis(grid[:, y0:y0 + s, x0:x0 + s], 0, -1).astype(np.float64)


def morton_xy(count):
    """(x, y) of the Morton indices 0..count-1: x takes the even bits"""
    i = np.arange(count)
    x = np.zeros(count, np.int64)
    y = np.zeros(count, np.int64)
    for b in range(8):
        x |= ((i >> (2 * b)) & 1) << b
        y |= ((i >> (2 * b + 1)) & 1) << b
    return x, y


# ---------------------------------------------------------------------------------------------------------------- frame and projection
def homography(src, tgt):
    """the 3x3 matrix (last entry 1) that maps the four 2-D points src onto tgt: the 8x8 system of the direct linear transform"""
    A = np.zeros((8, 8))
    A[:4, 0:2], A[:4, 2] = src, 1.0
    A[4:, 3:5], A[4:, 5] = src, 1.0
    A[:4, 6:8] = -src * tgt[:, 0:1]
    A[4:, 6:8] = -src * tgt[:, 1:2]
    h = np.linalg.solve(A, np.concatenate([tgt[:, 0], tgt[:, 1]]))
    return np.append(h, 1.0).reshape(3, 3)


def project(M, p):
    """homography M on (x, y) of the points p [..., 3]; z is kept"""
    q = np.concatenate([p[..., :2], np.ones(p.shape[:-1] + (1,))], -1) @ M.T
    return np.concatenate([q[..., :2] / q[..., 2:3], p[..., 2:3]], -1)


U = 2.0 ** -24  # unit roundoff of float32


def fp32_projection_error(P, S, M):
    """bound on |float32 projection - exact projection| of the vertices P [.., 3] under the frame S and the homography M, per axis (x, y, z), largest over the
    vertices: a three-term sum of products carries at most 3 u of the sum of its terms' magnitudes, u = 2^-24; the errors of the frame step enter the
    homography's sums through its coefficients; the division adds u of the quotient and divides both sums' errors by |w|."""
    aP = np.abs(P)
    dloc = 3 * U * (aP @ np.abs(S).T)  # [.., 3]
    loc = P @ S.T
    al = np.abs(loc)
    aM = np.abs(M)
    term = lambda k: 3 * U * (aM[k, 0] * al[..., 0] + aM[k, 1] * al[..., 1] + aM[k, 2]) + aM[k, 0] * dloc[..., 0] + aM[k, 1] * dloc[..., 1]
    w = np.abs(M[2, 0] * loc[..., 0] + M[2, 1] * loc[..., 1] + M[2, 2])
    q = project(M, loc)
    ex = (term(0) + np.abs(q[..., 0]) * term(2)) / w + U * np.abs(q[..., 0])
    ey = (term(1) + np.abs(q[..., 1]) * term(2)) / w + U * np.abs(q[..., 1])
    return np.array([ex.max(), ey.max(), dloc[..., 2].max()])


SQUARE = np.array([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0], [1.0, 1.0]])


def rect(lo, hi):
    return np.array([[lo[0], lo[1]], [hi[0], lo[1]], [lo[0], hi[1]], [hi[0], hi[1]]])


def frame(P, base=None):
    """(world [3,3] with the axes as columns, space = its inverse) of the blob's vertices P [row, column, xyz]: x along the mean of the two u edges,
    y along the mean of the two v edges of the corner quadrilateral, z their normal - not orthogonal in general.  base: the vertices the axes are
    taken from where they differ from P (leaf mode under displacement: the undisplaced surface)."""
    B = P if base is None else base
    f00, f10, f01, f11 = B[0, 0], B[0, -1], B[-1, 0], B[-1, -1]
    unit = lambda a: a / np.linalg.norm(a)
    vx = unit((f10 - f00) + (f11 - f01))
    vy = unit((f01 - f00) + (f11 - f10))
    vz = unit(np.cross(vx, vy))
    world = np.stack([vx, vy, vz], 1)
    return world, np.linalg.inv(world)


def alignment_margin(loc):
    """smallest of the differences the alignment check wants non-negative, over all cells: along every row x must not decrease, along every column y
    must not.  >= 0: aligned."""
    return min(float(np.diff(loc[..., 0], axis=1).min()), float(np.diff(loc[..., 1], axis=0).min()))


# ---------------------------------------------------------------------------------------------------------------- node planes
def plane_positions(plo, phi, clo, chi):
    """the ten normalised plane positions of nodes with parent boxes plo, phi [n, 3] and child boxes clo, chi [n, 4, 3] (children in Morton order: bit 0
    = right, bit 1 = upper), in the order of PLANES, [n, 10].  A border plane bounds the outer side of the two children on that side, measured from
    the parent's face on that side; a mid plane their inner side; the z planes all four.  A parent without extent gives position 0 (the encoder's scale
    for it is the smallest float)."""
    ext = phi - plo
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(ext > 0, 1.0 / ext, 0.0)
    left, right, low, up = [0, 2], [1, 3], [0, 1], [2, 3]
    out = np.stack([
        (clo[:, left, 0].min(1) - plo[:, 0]) * inv[:, 0], (clo[:, right, 0].min(1) - plo[:, 0]) * inv[:, 0],
        (phi[:, 0] - chi[:, left, 0].max(1)) * inv[:, 0], (phi[:, 0] - chi[:, right, 0].max(1)) * inv[:, 0],
        (clo[:, low, 1].min(1) - plo[:, 1]) * inv[:, 1], (clo[:, up, 1].min(1) - plo[:, 1]) * inv[:, 1],
        (phi[:, 1] - chi[:, low, 1].max(1)) * inv[:, 1], (phi[:, 1] - chi[:, up, 1].max(1)) * inv[:, 1],
        (clo[:, :, 2].min(1) - plo[:, 2]) * inv[:, 2], (phi[:, 2] - chi[:, :, 2].max(1)) * inv[:, 2]], 1)
    return out


def plane_extents(plo, phi):
    """the parent's extent along the axis of each of the ten planes, [n, 10]"""
    ext = phi - plo
    return ext[:, [0, 0, 0, 0, 1, 1, 1, 1, 2, 2]]


def table_index(pos):
    """[n, 10] positions -> the index of the largest table entry <= position (0 below the table), per plane"""
    return np.stack([np.clip(np.searchsorted(tab, pos[:, k], side="right") - 1, 0, len(tab) - 1) for k, (_, tab, _, _) in enumerate(PLANES)], 1)


def pack_words(idx):
    w = np.zeros(len(idx), np.uint32)
    for k, (_, _, sh, _) in enumerate(PLANES):
        w |= idx[:, k].astype(np.uint32) << np.uint32(sh)
    return w


def unpack_words(words):
    return np.stack([(words.astype(np.uint32) >> np.uint32(sh)) & np.uint32((1 << bits) - 1) for _, _, sh, bits in PLANES], 1).astype(np.int64)


def decode_children(idx, plo, phi, dtype=np.float64):
    """child boxes (lo, hi) [n, 4, 3] of nodes with plane indices idx [n, 10] and parent boxes plo, phi [n, 3]: table entry * extent + lower bound,
    rounded after the product and after the sum in `dtype` (float32: the encoder's and the kernels' own decode)."""
    f = dtype
    tb, tm, tz = T_BORDER.astype(f), T_MID.astype(f), T_Z.astype(f)
    plo, phi = plo.astype(f), phi.astype(f)
    dim = (phi - plo).astype(f)
    one = f(1.0)
    n = len(idx)
    mn = np.zeros((n, 4, 3), f)
    mx = np.zeros((n, 4, 3), f)
    for c in range(4):
        mn[:, c, 0] = tm[idx[:, 1]] if c & 1 else tb[idx[:, 0]]
        mx[:, c, 0] = one - tb[idx[:, 3]] if c & 1 else one - tm[idx[:, 2]]
        mn[:, c, 1] = tm[idx[:, 5]] if c & 2 else tb[idx[:, 4]]
        mx[:, c, 1] = one - tb[idx[:, 7]] if c & 2 else one - tm[idx[:, 6]]
        mn[:, c, 2] = tz[idx[:, 8]]
        mx[:, c, 2] = one - tz[idx[:, 9]]
    lo = ((mn * dim[:, None, :]).astype(f) + plo[:, None, :]).astype(f)
    hi = ((mx * dim[:, None, :]).astype(f) + plo[:, None, :]).astype(f)
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------- leaf heights
def plane_height(a, b, c, x, y):
    """z at (x, y) of the plane through the points a, b, c [n, 3]"""
    nrm = np.cross(b - a, c - a)
    with np.errstate(divide="ignore", invalid="ignore"):
        return a[:, 2] - (nrm[:, 0] * (x - a[:, 0]) + nrm[:, 1] * (y - a[:, 1])) / nrm[:, 2]


def corner_heights(q, lo, hi):
    """[n, 4]: the heights of a cell's height field at the four corners of its box (lo, hi [n, 3]), q [n, 4, 3] = the cell's projected vertices in grid
    order (row-major: (x,y), (x+1,y), (x,y+1), (x+1,y+1)).  The corner at (lo.x, lo.y) - lowerLeft - takes the plane through the three vertices that
    are not diagonally opposite to it in the grid, and so on: lowerRight at (hi.x, lo.y), upperLeft at (lo.x, hi.y), upperRight at (hi.x, hi.y)."""
    v1, v2, v3, v4 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([plane_height(v1, v2, v3, lo[:, 0], lo[:, 1]), plane_height(v1, v2, v4, hi[:, 0], lo[:, 1]),
                     plane_height(v1, v3, v4, lo[:, 0], hi[:, 1]), plane_height(v2, v3, v4, hi[:, 0], hi[:, 1])], 1)


def height_error(q, lo, hi, d):
    """[n, 4]: by how much a corner height of corner_heights() can move when the projected vertices deviate by up to d = (dx, dy, dz) per coordinate: the
    height is the combination of the three vertex heights with the barycentric weights of the corner, so a z deviation enters with the sum of the weights'
    magnitudes (1 inside the triangle, more where the corner lies outside it), an x or y deviation with that sum times the plane's slope along that axis.
    inf where the triangle is degenerate in the projection."""
    v1, v2, v3, v4 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    out = []
    for (a, b, c), x, y in (((v1, v2, v3), lo[:, 0], lo[:, 1]), ((v1, v2, v4), hi[:, 0], lo[:, 1]), ((v1, v3, v4), lo[:, 0], hi[:, 1]), ((v2, v3, v4), hi[:, 0], hi[:, 1])):
        nrm = np.cross(b - a, c - a)
        with np.errstate(divide="ignore", invalid="ignore"):
            wb = ((x - a[:, 0]) * (c[:, 1] - a[:, 1]) - (y - a[:, 1]) * (c[:, 0] - a[:, 0])) / nrm[:, 2]
            wc = ((b[:, 0] - a[:, 0]) * (y - a[:, 1]) - (b[:, 1] - a[:, 1]) * (x - a[:, 0])) / nrm[:, 2]
            s = (np.abs(1.0 - wb - wc) + np.abs(wb) + np.abs(wc)) * (d[2] + np.abs(nrm[:, 0] / nrm[:, 2]) * d[0] + np.abs(nrm[:, 1] / nrm[:, 2]) * d[1])
        out.append(np.where(np.isfinite(s), s, np.inf))
    return np.stack(out, 1)


def blob_extent(z, lo, hi):
    """how far the corner heights z [n, 4] leave the z range of their boxes, as a fraction of that range, largest over the cells, clamped to
    MAX_EXTENT; (clamped, unclamped).  Flat boxes do not take part."""
    zr = hi[:, 2] - lo[:, 2]
    out = np.maximum(np.maximum(z - hi[:, 2:3], 0.0), np.abs(np.minimum(z - lo[:, 2:3], 0.0))).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(zr != 0.0, out / zr, 0.0)
    raw = float(np.nanmax(np.append(rel, 0.0)))
    return min(raw, MAX_EXTENT), raw


def nibble_positions(z, lo, hi, extent):
    """[n, 4]: the corner heights on the scale of the 16 steps that span the box's z range widened by `extent` of itself on both sides; the stored
    nibble is floor() of this, clamped to 0..15.  NaN for flat boxes (their nibbles are 0)."""
    zr = hi[:, 2] - lo[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(zr[:, None] != 0.0, (z - (lo[:, 2] - extent * zr)[:, None]) * (16.0 / ((1.0 + 2.0 * extent) * zr))[:, None], np.nan)


def nibbles_of(pos):
    return np.where(np.isnan(pos), 0, np.clip(np.floor(np.nan_to_num(pos, nan=0.0, posinf=15.0, neginf=0.0)), 0, 15)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- bounds
def frustum_box(leaf_lo, leaf_hi, iproj):
    """box[0..9] of the header: the z range of the decoded cells, then (x, y) in the blob's frame of four corners of their bounding box taken back through
    the projection: lower-left and lower-right at the lower z, upper-left and upper-right at the upper z"""
    lo, hi = leaf_lo.min(0), leaf_hi.max(0)
    c = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [lo[0], hi[1], hi[2]], [hi[0], hi[1], hi[2]]])
    return np.concatenate([[lo[2], hi[2]], project(iproj, c)[:, :2].ravel()])


def world_bounds(leaf_lo, leaf_hi, iproj, world):
    """(wlo, whi): every decoded cell box is taken back through the projection corner by corner, bounded in the blob's frame, and seven of that box's
    eight corners are taken to world space - the reference's list, in which (lx, ly, uz) is absent and (ux, uy, uz) appears twice"""
    n = len(leaf_lo)
    b = np.stack([leaf_lo, leaf_hi], 1)  # [n, 2, 3]
    sel = np.array([[i, j, k] for k in (0, 1) for j in (0, 1) for i in (0, 1)])
    corners = np.stack([b[:, sel[:, 0], 0], b[:, sel[:, 1], 1], b[:, sel[:, 2], 2]], -1)  # [n, 8, 3]
    loc = project(iproj, corners)
    t = np.stack([loc.min(1), loc.max(1)], 1)
    keep = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]])
    pts = np.stack([t[:, keep[:, 0], 0], t[:, keep[:, 1], 1], t[:, keep[:, 2], 2]], -1).reshape(n * 7, 3)
    w = pts @ world.T
    return w.min(0), w.max(0)


# ---------------------------------------------------------------------------------------------------------------- the blob
def ref_blob(P, C, mode, words=None, base=None):
    """The float64 derivation of one blob from its (2^C+1)^2 kept vertices P [row, column, xyz] (window()); mode 'box' | 'leaf' | 'grid' | 'full'.

    1. frame(): axes from the corner vertices; loc = the vertices in that frame.
    2. Alignment (box, leaf, full; grid never): aligned iff along every grid row loc.x and along every grid column loc.y never decrease, and the
       homography that takes the four corner vertices' (x, y) onto the square [-1,1]^2 leaves every vertex finite and within [-1.5, 1.5]^2.  Aligned:
       that homography, followed by the affine map that takes the bounding rectangle of the projected vertices onto the square.  Otherwise
       (the fallback): the affine map of the bounding rectangle of loc onto the square.  z is never projected.
    3. Every cell's box = the bounds of its four projected vertices, cells in Morton order, merged four by four up to the root.
    4. Top-down, each node stores for its four children ten planes as indices into three tables (largest entry <= the normalised position, measured
       inwards from the parent's faces); the children are then REPLACED by what those indices decode to, so that the next level is measured against
       the boxes a ray will see.  `words` given (the product's, [elems] uint32): the chain is decoded from them instead of from the indices derived
       here, in float32 like the encoder's; both sets of indices are returned.  full mode stores the float boxes and replaces nothing.
    5. leaf mode: per cell the heights of its surface at the four corners of its DECODED box, the blob's extent from how far they leave the box, and
       4-bit positions of the heights in the widened range.
    6. frustum box and world bounds from the decoded cells.

    Returns a dict: world, space, proj, iproj, loc, pv (projected vertices [row, column, 3]), aligned, margin (of the verdict: alignment_margin, or
    the distance to 1.5 where that decided; |margin| small = a tie), flat (z range of pv exactly 0), hier (list per level 0..C of (lo, hi) in Morton
    order, undecoded), pos (list per level 0..C-1 of [n, 10] positions against the chain's parents), idx (the indices derived from pos), used (the
    indices the chain was decoded with), parents (list per level of (lo, hi) the nodes were measured against), cells (lo, hi: decoded cell boxes),
    heights [cells, 4], extent, extent_raw, nibpos [cells, 4], box [10], wlo, whi."""
    s = 2 ** C + 1
    assert P.shape == (s, s, 3)
    world, space = frame(P, base)
    loc = P @ space.T
    flatv = loc.reshape(-1, 3)
    llo, lhi = flatv.min(0), flatv.max(0)
    scale = max(1.0, float(np.abs(flatv[:, :2]).max()))
    margin = alignment_margin(loc) / scale
    aligned = mode != "grid" and margin >= 0.0
    if mode == "grid":
        margin = -np.inf
    proj = None
    if aligned:
        h1 = homography(np.array([loc[0, 0, :2], loc[0, -1, :2], loc[-1, 0, :2], loc[-1, -1, :2]]), SQUARE)
        p1 = project(h1, loc)
        xy = p1[..., :2]
        m2 = float((1.5 - np.abs(xy)).min()) if np.isfinite(xy).all() else -np.inf
        margin = min(margin, m2)
        if m2 < 0.0:
            aligned = False
        else:
            q = xy.reshape(-1, 2)
            proj = homography(rect(q.min(0), q.max(0)), SQUARE) @ h1
    if not aligned:
        proj = homography(rect(llo, lhi), SQUARE)
    iproj = np.linalg.inv(proj)
    pv = project(proj, loc)

    ncell = 4 ** C
    mx, my = morton_xy(ncell)
    quad = np.stack([pv[my, mx], pv[my, mx + 1], pv[my + 1, mx], pv[my + 1, mx + 1]], 1)  # [cells, 4, 3]
    hier = [None] * (C + 1)
    hier[C] = (quad.min(1), quad.max(1))
    for l in range(C - 1, -1, -1):
        lo, hi = hier[l + 1]
        hier[l] = (lo.reshape(-1, 4, 3).min(1), hi.reshape(-1, 4, 3).max(1))

    pos, idx, used, parents = [], [], [], []
    plo, phi = hier[0]
    off = 0
    for l in range(C):
        clo, chi = hier[l + 1]
        clo, chi = clo.reshape(-1, 4, 3), chi.reshape(-1, 4, 3)
        parents.append((plo, phi))
        n = len(plo)
        if mode == "full":
            plo, phi = clo.reshape(-1, 3), chi.reshape(-1, 3)
            continue
        p = plane_positions(np.asarray(plo, np.float64), np.asarray(phi, np.float64), clo, chi)
        i = table_index(p)
        pos.append(p)
        idx.append(i)
        if words is None:
            u = i
            dlo, dhi = decode_children(u, plo, phi)
        else:
            u = unpack_words(words[off:off + n])
            dlo, dhi = decode_children(u, plo.astype(np.float32), phi.astype(np.float32), np.float32)
        used.append(u)
        off += n
        plo, phi = dlo.reshape(-1, 3), dhi.reshape(-1, 3)
    cell_lo, cell_hi = np.asarray(plo, np.float64), np.asarray(phi, np.float64)

    out = dict(world=world, space=space, proj=proj, iproj=iproj, loc=loc, pv=pv, aligned=aligned, margin=margin, flat=bool(hier[0][0][0, 2] == hier[0][1][0, 2]),
               hier=hier, pos=pos, idx=idx, used=used, parents=parents, cells=(cell_lo, cell_hi), quad=quad)
    if mode == "leaf":
        z = corner_heights(quad, cell_lo, cell_hi)
        ext, raw = blob_extent(z, cell_lo, cell_hi)
        out.update(heights=z, extent=ext, extent_raw=raw, nibpos=nibble_positions(z, cell_lo, cell_hi, ext))
    else:
        out.update(heights=None, extent=0.0, extent_raw=0.0, nibpos=None)
    out["box"] = frustum_box(cell_lo, cell_hi, iproj)
    out["wlo"], out["whi"] = world_bounds(cell_lo, cell_hi, iproj, world)
    return out


# ---------------------------------------------------------------------------------------------------------------- brute force
def triangles_of(grids, diagonal="product"):
    """(a, b, c [n, 3] float64, patch ID [n]) of the two triangles of every cell of the kept grids.

    diagonal="product": a cell with the vertices v00 (x, y), v10 (x+1, y), v01 (x, y+1), v11 (x+1, y+1) is split along v10 - v01 into (v00, v10, v01) and
    (v01, v10, v11): the split of the eager leaf (GridCell in csrc/accel.h: vertex p[3 r + c]; the vertex nibbles of GridCellLeaf in
    csrc/trace_grid.hip.h give the triangles (0,1,3) (3,1,4) ... of the 3x3 cell, i.e. the reference's Gather3x3) and of bvh4.compressed.grid.
    diagonal="other": along v00 - v11."""
    A, B, Cc, ids = [], [], [], []
    for pid in sorted(grids):
        g = np.moveaxis(np.asarray(grids[pid], np.float64), 0, -1)
        v00, v10, v01, v11 = g[:-1, :-1].reshape(-1, 3), g[:-1, 1:].reshape(-1, 3), g[1:, :-1].reshape(-1, 3), g[1:, 1:].reshape(-1, 3)
        if diagonal == "product":
            tri = ((v00, v10, v01), (v01, v10, v11))
        else:
            assert diagonal == "other"
            tri = ((v00, v10, v11), (v00, v11, v01))
        for a, b, c in tri:
            A.append(a), B.append(b), Cc.append(c), ids.append(np.full(len(a), pid, np.int64))
    return np.concatenate(A), np.concatenate(B), np.concatenate(Cc), np.concatenate(ids)


def brute_force(rays, grids, diagonal="product", chunk=512):
    """Closest hit of every ray, in float64, over both triangles of every cell of the kept grids (the Moeller-Trumbore quantities, every ray against every
    triangle, as matrix products in chunks of `chunk` rays: 512 rays x 4096 triangles x ten float64 arrays stay below 200 MB).  tnear < t <= tfar as the records give them.
    Returns (t [n] float64, inf for a miss; patch ID [n] int64, -1 for a miss; margin [n]: the smallest of the hit's barycentric coordinates u, v, 1-u-v,
    i.e. its distance from the triangle's border in units of the triangle - inf for a miss)."""
    a, b, c, ids = triangles_of(grids, diagonal)
    e1, e2 = b - a, c - a
    # with tvec = o - a and m = o x d the triple products separate into a part per ray times a part per triangle:
    #   det = e1 . (d x e2) = -d . n,  n = e1 x e2;   t det = tvec . n;   u det = e2 . (tvec x d) = m . e2 - d . (e2 x a);   v det = -e1 . (tvec x d)
    nrm = np.cross(e1, e2)
    an = (a * nrm).sum(1)
    e2a, e1a = np.cross(e2, a), np.cross(e1, a)
    org = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1).astype(np.float64)
    drc = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1).astype(np.float64)
    mom = np.cross(org, drc)
    tn, tf = rays["tnear"].astype(np.float64), rays["tfar"].astype(np.float64)
    n = len(org)
    T = np.full(n, np.inf)
    ID = np.full(n, -1, np.int64)
    MG = np.full(n, np.inf)
    for s in range(0, n, chunk):
        o, d, m = org[s:s + chunk], drc[s:s + chunk], mom[s:s + chunk]
        det = -(d @ nrm.T)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            t = (o @ nrm.T - an[None]) * inv
            u = (m @ e2.T - d @ e2a.T) * inv
            v = -(m @ e1.T - d @ e1a.T) * inv
        mg = np.minimum(np.minimum(u, v), 1.0 - u - v)
        ok = (det != 0.0) & (mg >= 0.0) & (t > tn[s:s + chunk, None]) & (t <= tf[s:s + chunk, None])
        t = np.where(ok, t, np.inf)
        k = t.argmin(1)
        r = np.arange(len(k))
        hit = np.isfinite(t[r, k])
        T[s:s + chunk] = t[r, k]
        ID[s:s + chunk] = np.where(hit, ids[k], -1)
        MG[s:s + chunk] = np.where(hit, mg[r, k], np.inf)
    return T, ID, MG


# ---------------------------------------------------------------------------------------------------------------- rays against the truth
RAY_CASES = (("bomb32", 2, 1), ("bomb32", 3, 2), ("bomb32", 3, 3), ("fallback", 3, 3))  # (mesh, L, C); deeper pairs add no code path, only triangles
RAY_MODES = ("default", "bvh4.compressed.box", "bvh4.compressed.leaf", "bvh4.compressed.grid", "bvh4.compressed.full")
MARGIN = 1e-6      # a truth hit closer than this to its triangle's border (barycentric) may be set aside ...
MARGIN_CAP = 1e-3  # ... at most this share of the truth hits
FARTHER = 1e-3     # relative; a hit reported farther than the true surface by more than this is "behind the surface"
FLIPS = 2          # the hit/miss allowance of the parity tests (helpers.check_fork_parity)
# Measured on the oracle alone in product arithmetic (tests/test_host_cbvh_ray_truth.py asserts them; tests/test_gpu_cbvh_truth.py holds the kernels to the
# truth with them): truth = rays the brute force hits; per mode (hits, farther, nearer, largest relative error of t on common hits - eager / grid only).
# lost is 0 everywhere and added = hits - truth.  `farther` of the 32-face mesh is bounded by FLIPS whatever was measured (0 or 1).  On fallback_mesh()
# box / leaf / full report 4 / 48 / 2 hits behind the surface: every one of them has its true hit in a blob that took the affine fallback, where the surface
# folds over itself in the blob's frame and is no height field (the leaf mode's extent estimate is 12 to 700 there and is clamped to 1, so the 4-bit heights
# cannot reach the surface; box and full report box entry points of cells that overlap in the projection).  That is the fork's algorithm, not the encoding:
# the counts are pinned and capped at measured + FLIPS, and the test asserts the cause (no such hit in an aligned blob beyond FLIPS).
PINNED = {
    ("bomb32", 2, 1): dict(truth=2402, default=(2402, 0, 0, 4.41e-7), box=(2571, 0, 11, None), leaf=(2570, 0, 2, None), grid=(2402, 0, 0, 2.43e-7), full=(2571, 0, 11, None)),
    ("bomb32", 3, 2): dict(truth=2438, default=(2438, 0, 0, 2.21e-7), box=(2571, 0, 13, None), leaf=(2570, 0, 3, None), grid=(2438, 0, 0, 2.92e-7), full=(2526, 0, 7, None)),
    ("bomb32", 3, 3): dict(truth=2438, default=(2438, 0, 0, 2.21e-7), box=(2983, 1, 48, None), leaf=(2980, 1, 9, None), grid=(2438, 0, 0, 2.92e-7), full=(2664, 0, 17, None)),
    ("fallback", 3, 3): dict(truth=9092, default=(9092, 0, 0, 1.32e-6), box=(12221, 4, 6645, None), leaf=(10721, 48, 6348, None), grid=(9092, 0, 0, 3.00e-6), full=(10163, 2, 6445, None)),
}

_truth_cache = {}


def named_mesh(bomberman, name):
    import cbvh_forms_helpers as cf
    return cf.mesh(bomberman) if name == "bomb32" else fallback_mesh()


def ray_truth(rtc, po, bomberman, mesh, L, C):
    """(mesh, the 20 000 RTCRayHit records of the form matrix's generator through the mesh's bounding box, t, patch ID, margin of brute_force(), {patch ID:
    aligned} of the blobs at L == C else None); computed once per process.  The vertex grids come from a host-only device."""
    import cbvh_forms_helpers as cf
    key = (mesh, L, C)
    if key not in _truth_cache:
        m = named_mesh(bomberman, mesh)
        src = cf.make_rays(po, m[0])
        dev = rtc.Device("gpu=none,keep_grids=1")
        sc = rtc.Scene(dev)
        assert sc.add_subdiv(*m) == 0
        sc.set_levels(L, C)
        sc.commit()
        grids = {k: v.copy() for k, v in kept_grids(sc, L).items()}
        sc.release()
        dev.release()
        t, pid, mg = brute_force(src, grids)
        aligned = {p: ref_blob(window(g, 0, 0, C), C, "box")["aligned"] for p, g in grids.items()} if L == C else None
        for a in (t, pid, mg):
            a.setflags(write=False)
        src.setflags(write=False)
        _truth_cache[key] = (m, src, t, pid, mg, aligned)
    return _truth_cache[key]


def truth_stats(rec, t, pid, mg):
    """traced RTCRayHit records against the truth.  A ray whose truth hit lies within MARGIN of its triangle's border is set aside where it disagrees in hit /
    miss or patch ID (it counts in `aside`, not in lost / added / ids)."""
    hit = rec["geomID"] != 0xFFFFFFFF
    th_ = np.isfinite(t)
    edge = th_ & (mg < MARGIN)
    both = hit & th_
    wrong_id = both & (rec["primID"].astype(np.int64) != pid)
    lost, added = th_ & ~hit, hit & ~th_
    aside = edge & (lost | wrong_id)
    same = both & ~aside
    rel = (rec["tfar"][same].astype(np.float64) - t[same]) / t[same]
    far = np.zeros(len(t), bool)
    far[np.nonzero(same)[0][rel > FARTHER]] = True
    return dict(truth=int(th_.sum()), hits=int(hit.sum()), lost=int((lost & ~aside).sum()), added=int(added.sum()), ids=int((wrong_id & ~aside).sum()),
                aside=int(aside.sum()), farther=int(far.sum()), nearer=int((rel < -FARTHER).sum()), maxrel=float(np.abs(rel).max()) if rel.size else 0.0, far_rays=far)
