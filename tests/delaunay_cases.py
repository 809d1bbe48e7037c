"""Inputs and the independent checker of the lattice Delaunay / Mesh-MNIST maker tests (tests/test_delaunay*.py,
tests/test_mesh_digits*.py).  Everything comes from fixed seeds; predicates are Python-int arithmetic written here, not taken from
the package."""
import numpy as np

M24 = (1 << 24) - 1


def orient(a, b, c):
    return (int(b[0]) - int(a[0])) * (int(c[1]) - int(a[1])) - (int(b[1]) - int(a[1])) * (int(c[0]) - int(a[0]))


def incircle(a, b, c, d):
    rows = [(int(p[0]) - int(d[0]), int(p[1]) - int(d[1])) for p in (a, b, c)]
    (ax, ay), (bx, by), (cx, cy) = rows
    al, bl, cl = ax * ax + ay * ay, bx * bx + by * by, cx * cx + cy * cy
    return ax * (by * cl - bl * cy) - ay * (bx * cl - bl * cx) + al * (bx * cy - by * cx)


def hull_with_collinear(P):
    """Indices of every point on the boundary of the convex hull (points inside hull edges included).  Not all collinear."""
    idx = sorted(range(len(P)), key=lambda i: (int(P[i][0]), int(P[i][1])))

    def chain(seq):
        h = []
        for i in seq:
            while len(h) >= 2 and orient(P[h[-2]], P[h[-1]], P[i]) < 0:
                h.pop()
            h.append(i)
        return h
    return set(chain(idx)) | set(chain(idx[::-1]))


def check_triangulation(P, F):
    """Asserts that F is a Delaunay triangulation of the convex hull of P in the sense of include/sn_spmm.h; returns
    (cocircular, boundary vertices)."""
    P = [(int(x), int(y)) for x, y in np.asarray(P).tolist()]
    F = [tuple(int(v) for v in f) for f in np.asarray(F).tolist()]
    n = len(P)
    across = {}
    for a, b, c in F:
        assert len({a, b, c}) == 3 and min(a, b, c) >= 0 and max(a, b, c) < n
        assert orient(P[a], P[b], P[c]) > 0, "a face is not counter-clockwise with non-zero area"
        for u, v, w in ((a, b, c), (b, c, a), (c, a, b)):
            assert (u, v) not in across, "an edge has more than two faces, or two faces on one side"
            across[(u, v)] = w
    cocircular = 0
    out = {}
    for (u, v), w in across.items():
        if (v, u) in across:
            val = incircle(P[u], P[v], P[w], P[across[(v, u)]])
            assert val <= 0, "an interior edge is not locally Delaunay"
            cocircular += val == 0
        else:
            assert u not in out, "the boundary is not one simple ring"
            out[u] = v
    assert cocircular % 2 == 0
    boundary = set(out)
    assert boundary == set(out.values())
    v0 = next(iter(out))                            # one ring through every boundary vertex
    v, steps = out[v0], 1
    while v != v0:
        v, steps = out[v], steps + 1
        assert steps <= n
    assert steps == len(boundary)
    assert len(F) == 2 * n - 2 - len(boundary), "nF != 2 n - 2 - b"
    assert {v for f in F for v in f} == set(range(n)), "a point is not a vertex"
    assert boundary == hull_with_collinear(P), "the boundary is not the convex hull with its collinear points"
    return cocircular // 2, len(boundary)


def has_collinear_hull_triple(P):
    P = [(int(x), int(y)) for x, y in np.asarray(P).tolist()]
    H = hull_with_collinear(P)
    strict = []
    for seq in (sorted(H, key=lambda i: P[i]), sorted(H, key=lambda i: P[i], reverse=True)):
        h = []
        for i in seq:
            while len(h) >= 2 and orient(P[h[-2]], P[h[-1]], P[i]) <= 0:
                h.pop()
            h.append(i)
        strict += h
    return set(strict) != H


def random_set(n, seed, span=1 << 20):
    rng = np.random.default_rng(seed)
    while True:
        P = rng.integers(-span, span, size=(n, 2)).astype(np.int32)
        if len({(int(x), int(y)) for x, y in P}) == n:
            return P


def general_position_cases(max_points):
    """name -> (n, 2) int32; every one has cocircular == 0 and no collinear hull triple (asserted by the tests)."""
    big = 9_000_000
    return {
        "n3": np.array([[0, 0], [7, 1], [2, 9]], np.int32),
        "n4_convex": np.array([[0, 0], [10, 1], [12, 11], [-1, 8]], np.int32),
        "n4_inside": np.array([[0, 0], [30, 2], [11, 29], [13, 9]], np.int32),
        "random5": random_set(5, 11),
        "random50": random_set(50, 12),
        "random210": random_set(210, 13, 27 << 15) + np.int32(27 << 15),
        "random_max": random_set(max_points, 14, 1 << 23),
        "max_magnitude": np.array([[-M24, -M24], [M24, -M24], [0, M24], [M24, M24]], np.int32),
        "max_magnitude_in": np.array([[-M24, -M24], [M24, -M24], [1, M24], [M24, M24 - 1]], np.int32),
        "max_magnitude_out": np.array([[-M24 + 1, -M24], [M24, -M24], [0, M24 - 1], [M24, M24]], np.int32),
        "far_corner": random_set(40, 15, 1000) + np.int32(big),
    }


def collinear_prefix_cases():
    """Three points share the smallest x: the sweep starts with a collinear chain.  The hull has a collinear triple, the interior
    is in general position (cocircular == 0 is asserted)."""
    return {
        "prefix3": np.array([[-5, 0], [-5, 7], [-5, 19], [3, 4], [9, 15], [14, -2], [6, 8]], np.int32),
        "prefix3_right": np.array([[-5, 19], [4, -30], [-5, 0], [-5, 7], [2, 3], [11, 5]], np.int32),
        "prefix_then_line": np.array([[0, 0], [0, 5], [0, 9], [0, 14], [4, 28], [3, 7], [8, 42]], np.int32),
    }


PYTHAGOREAN = [(3, 4), (-3, 4), (3, -4), (-3, -4), (4, 3), (-4, 3), (4, -3), (-4, -3), (5, 0), (-5, 0), (0, 5), (0, -5)]


def pythagorean_circle(k=1000, shift=(8_000_000, -7_000_000)):
    return np.array([(x * k + shift[0], y * k + shift[1]) for x, y in PYTHAGOREAN], np.int32)


def near_cocircular_quads(k=1000, shift=(8_000_000, -7_000_000)):
    """Four points of the circle, A = (5k, 0) moved one lattice unit inwards and outwards: (P_in, P_out); A is index 0, the point
    opposite to it index 2.  Inwards A lies inside the circle of the others, so the diagonal is 0-2; outwards it is 1-3."""
    base = [(5 * k, 0), (3 * k, 4 * k), (-4 * k, 3 * k), (0, -5 * k)]
    out = []
    for d in (-1, 1):
        q = [(base[0][0] + d, base[0][1])] + base[1:]
        out.append(np.array([(x + shift[0], y + shift[1]) for x, y in q], np.int32))
    return out


def near_cocircular_dozen():
    """The twelve circle points with one moved inwards / outwards: the other eleven stay cocircular."""
    out = []
    for d in (-1, 1):
        P = pythagorean_circle()
        P[8, 0] += d
        out.append(P)
    return out


def degenerate_valid_cases():
    """Cocircular everywhere and / or collinear hulls: any valid triangulation is accepted, cocircular > 0."""
    grid = lambda w, h, s, o: np.array([(o + s * x, o - 3 + s * y) for x in range(w) for y in range(h)], np.int32)
    return {
        "grid4x4": grid(4, 4, 17, 100),
        "grid5x3": grid(5, 3, 1 << 18, -(1 << 20)),
        "square": np.array([[0, 0], [64, 0], [64, 64], [0, 64]], np.int32) + np.int32(5000),
        "dozen": pythagorean_circle(),
    }


def pad_batch(sets, nmax=None):
    nmax = max(len(s) for s in sets) if nmax is None else nmax
    P = np.zeros((len(sets), nmax, 2), np.int32)
    for i, s in enumerate(sets):
        P[i, : len(s)] = s
    return P, np.array([len(s) for s in sets], np.int32)


def ragged_refusal_batch(max_points):
    """(sets, expected status bit or 0) of the mixed batch: counts 0, 1, 2, 3, a collinear set, a duplicate, a coordinate out of
    range, one point too many, two good sets."""
    from surfacenetworks_amd import mesh_ops as mo

    line = np.array([(3 * i, 5 * i - 2) for i in range(9)], np.int32)
    dup = random_set(20, 21)
    dup[13] = dup[4]
    far = random_set(12, 22)
    far[5, 1] = 1 << 24
    too = random_set(max_points + 1, 23, 1 << 23)
    sets = [np.zeros((0, 2), np.int32), random_set(1, 24), random_set(2, 25), random_set(3, 26), line, dup, far, too,
            random_set(64, 27), random_set(210, 28)]
    want = [mo.DT_DEGENERATE, mo.DT_DEGENERATE, mo.DT_DEGENERATE, 0, mo.DT_DEGENERATE, mo.DT_DUPLICATE, mo.DT_RANGE,
            mo.DT_TOO_LARGE, 0, 0]
    return sets, want


def stroke_images(count=6, size=28, seed=5):
    """Synthetic uint8 digits: seeded thick strokes; image 0 is all zero, image 1 all 255."""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, size, size), np.uint8)
    yy, xx = np.mgrid[0:size, 0:size]
    for b in range(2, count):
        img = np.zeros((size, size))
        for _ in range(3):
            (x0, y0), (x1, y1) = rng.uniform(0.15 * size, 0.85 * size, size=(2, 2))
            t = np.clip(((xx - x0) * (x1 - x0) + (yy - y0) * (y1 - y0)) / max((x1 - x0) ** 2 + (y1 - y0) ** 2, 1e-9), 0, 1)
            d2 = (xx - x0 - t * (x1 - x0)) ** 2 + (yy - y0 - t * (y1 - y0)) ** 2
            img = np.maximum(img, np.exp(-d2 / (2 * (0.045 * size) ** 2)))
        out[b] = np.rint(255 * img).astype(np.uint8)
    if count > 1:
        out[1] = 255
    return out
