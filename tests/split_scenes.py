"""The hand-made scenes of the pre-splitting tests (tests/test_np_split.py on the host, tests/test_gpu_split_refs.py on the device): the
smallest triangle lists on which each arm of the splitter is live.  Every scene is (vertices [3n, 3] float32, object-to-world matrix 4x4
row-major or None), one instance, generated from seeds."""
import numpy as np

BUDGETS = (10, 30, 100)
BOTH_TESTS = ("grid8", "far")  # the scenes that run with both VKRT_OPT_WATERTIGHT values


def _tris(*t):
    return np.array(t, np.float32).reshape(-1, 3)


def _small(rng, n, lo, hi, size):
    p0 = rng.uniform(lo, hi, (n, 1, 3))
    return (p0 + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 3)


def _anchors(a=0.0, b=8.0):
    """Two small right triangles in opposite corners: the scene bounds are exactly [a, b]^3."""
    d = (b - a) / 32
    return _tris([a, a, a], [a + d, a, a], [a, a + d, a], [b, b, b], [b - d, b, b], [b, b - d, b])


def grid8():
    """Scene bounds [0, 8]^3, so every median plane is a binary fraction: vertices exactly on the planes x = 4, y = 2 and z = 6 (the
    da <= pos and da >= pos arms together), triangles inside one plane, two wall triangles with a zero-thickness box, one large diagonal
    triangle (id 12) that takes the largest share of the budget, 60 fillers."""
    rng = np.random.default_rng(801)
    on_planes = _tris([4, 1, 1], [1, 5, 3], [7, 3, 5],          # a vertex on x = 4, the first plane of its box
                      [1, 2, 1], [7, 0.5, 3], [6, 3.5, 7],      # a vertex on y = 2
                      [1, 1, 6], [3, 7, 5], [2, 4, 7.5],        # a vertex on z = 6
                      [4, 2, 6], [1.5, 0.5, 2.5], [6.5, 5, 7],  # a vertex on all three
                      [4, 0.5, 0.5], [4, 7, 2], [0.5, 3, 7])    # an edge inside x = 4: two vertices on the plane
    in_plane = _tris([4, 1, 1], [4, 6, 2], [4, 3, 7],           # all of it inside x = 4
                     [1, 1, 6], [7, 2, 6], [3, 7, 6],           # inside z = 6
                     [0.5, 2, 0.5], [7, 2, 1], [2, 2, 7.5])     # inside y = 2
    walls = _tris([0.5, 0.5, 3], [7.5, 0.5, 3], [7.5, 7.5, 3], [0.5, 0.5, 3], [7.5, 7.5, 3], [0.5, 7.5, 3])
    diagonal = _tris([0.25, 0.375, 0.125], [7.75, 7.625, 0.875], [0.625, 7.5, 7.875])
    return np.concatenate([_anchors(), on_planes, in_plane, walls, diagonal, _small(rng, 60, 0.5, 7.5, 0.15)]).astype(np.float32), None


def one_giant():
    """300 tiny triangles and one room-sized diagonal triangle: at budget 100 its splits reach the cap of 255."""
    rng = np.random.default_rng(802)
    giant = _tris([0.1, 0.2, 0.3], [9.7, 9.1, 1.3], [5.3, 0.4, 9.9])
    return np.concatenate([_small(rng, 300, 0.5, 9.5, 0.004), giant]).astype(np.float32), None


def needles_and_lines():
    """Needles (slop > 0: priority 0, whole), exactly collinear triangles (zero area and zero slop, but a box with positive area: split
    into segments), repeated vertices, among ordinary triangles."""
    rng = np.random.default_rng(803)
    n = 40
    p0 = rng.uniform(1, 9, (n, 3))
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = rng.standard_normal((n, 3))
    t -= (t * d).sum(1, keepdims=True) * d
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    phi = rng.uniform(1e-4, 0.05, n)[:, None]
    ln = rng.uniform(2, 6, (n, 1))
    needles = np.stack([p0, p0 + ln * d, p0 + ln * (np.cos(phi) * d + np.sin(phi) * t)], 1).reshape(-1, 3)
    # e2 = 3 e1 exactly in binary32, with either record format: all coordinates are small multiples of 1/2
    a = np.array([[1, 1, 1], [2, 7, 1.5], [8, 2, 6], [0.5, 9, 9], [3, 3, 0.5], [9, 1, 1]], np.float32)
    e = np.array([[1, 0.5, 2], [1.5, -1, 2], [-2, 2, -1.5], [2.5, -2.5, -2.5], [2, 0, 3], [-2.5, 2.5, 2.5]], np.float32)
    lines = np.stack([a, a + e, a + 3 * e], 1).reshape(-1, 3)
    repeated = _tris([1, 8, 2], [1, 8, 2], [7, 3, 9], [2, 2, 8], [9, 7, 1], [9, 7, 1], [5, 5, 5], [5, 5, 5], [5, 5, 5])
    return np.concatenate([_anchors(0.0, 10.0), needles, lines, repeated, _small(rng, 120, 0.5, 9.5, 0.4)]).astype(np.float32), None


def far():
    """A 2 mm soup at 1e5 (tests/test_gpu_bvh_bounds.py: soup_far) and three triangles large against the scene grid: the spacing of
    binary32 is 2^-7 there and the 8-ulp pad of a cut point a visible fraction of a piece."""
    from test_gpu_bvh_bounds import _soup

    rng = np.random.default_rng(804)
    big = np.concatenate([s * rng.uniform(-1, 1, (3, 3)) for s in (2e3, 5e3, 2e4)])
    world = np.diag([1e-4, 1e-4, 1e-4, 1.0])
    world[:3, 3] = 1e5
    return np.concatenate([_soup(400), big]).astype(np.float32), world


def flat():
    """Every triangle inside z = 0, with a right angle at its first vertex (no slop): the grid has no extent on one axis."""
    rng = np.random.default_rng(805)
    n = 208
    p0 = np.concatenate([rng.uniform(1, 9, (200, 2)), rng.uniform(3, 7, (8, 2))])
    a = rng.uniform(0, 2 * np.pi, n)
    la, lb = np.concatenate([rng.uniform(0.1, 0.5, (200, 2)), rng.uniform(2, 3, (8, 2))]).T
    p = np.zeros((n, 3, 3))
    p[:, :, :2] = p0[:, None]
    p[:, 1, :2] += la[:, None] * np.stack([np.cos(a), np.sin(a)], 1)
    p[:, 2, :2] += lb[:, None] * np.stack([-np.sin(a), np.cos(a)], 1)
    return p.reshape(-1, 3).astype(np.float32), None


def soup(n):
    """_soup(n) with ten triangles enlarged tenfold about their first vertex: across the 1024-thread stride of k_split_budget (n = 1025)
    and the 256-thread blocks (n = 257)."""
    from test_gpu_bvh_bounds import _soup

    p = _soup(n).reshape(-1, 3, 3)
    big = np.arange(10) * (n // 10)
    p[big, 1:] = p[big, :1] + 10 * (p[big, 1:] - p[big, :1])
    return p.reshape(-1, 3).astype(np.float32), None


HAND_MADE = {"grid8": grid8, "one_giant": one_giant, "needles_and_lines": needles_and_lines, "far": far, "flat": flat,
             "soup1025": lambda: soup(1025), "soup257": lambda: soup(257)}
