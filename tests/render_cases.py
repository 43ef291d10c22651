"""The shared case list of the render tests (a helper, not collected): every case is built from a seed, the smallest
shapes at which the kernels of csrc/render.hip can still go wrong.  test_render.py holds the numpy twins to a plain
Python loop on these cases, test_render_gpu.py holds the device to the twins."""
import numpy as np

from softgroup_amd.ops import render as RO
from softgroup_amd.ops.render import Camera
from softgroup_amd.util import render as UR

EYE3 = np.eye(3)
DOWN = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])      # rows (right, up, forward): straight down
F32 = np.float32


def case(name, coords, cams, width, height, point_size=0, world_radius=None):
    coords = np.ascontiguousarray(np.asarray(coords, F32).reshape(-1, 3))
    return dict(name=name, coords=coords, cams=RO.camera_table(cams), width=width, height=height,
                point_size=point_size, world_radius=world_radius)


def persp(width, height, f=None, near=0.5, far=None, eye=(0.0, 0.0, 0.0)):
    """looks along +z from the eye: zc = double(z) - ez exactly"""
    return Camera('perspective', eye, EYE3, width / 2 if f is None else f, width / 2, height / 2, near, far)


def ortho(width, height, f=1.0, near=None, far=None, eye=(0.0, 0.0, 0.0), rot=EYE3):
    return Camera('orthographic', eye, rot, f, width / 2, height / 2, near, far)


def at_pixel(cam, u, v, z):
    """the point that a `persp` / `ortho` camera with the identity rotation and the eye at the origin sees at (u, v)"""
    s = z / cam.f if cam.kind == 'perspective' else 1.0 / cam.f
    return [(u - cam.cx) * s, -(v - cam.cy) * s, z]


def scatter(seed, n, width, height, point_size):
    """n points over the image and three pixels beyond it on every side, with points on the four borders and in the
    four corners in front of everything else: splats clipped on every side and on two sides at once"""
    rng = np.random.default_rng(seed)
    cam = persp(width, height)
    pts = [at_pixel(cam, u, v, 0.9) for u in (0.3, width - 0.3) for v in (0.3, height - 0.3)]
    pts += [at_pixel(cam, u, height / 2 + 0.4, 0.9) for u in (0.3, width - 0.3)]
    pts += [at_pixel(cam, width / 2 + 0.4, v, 0.9) for v in (0.3, height - 0.3)]
    pts += [at_pixel(cam, u, v, 0.95) for u, v in ((-1.5, -1.5), (width + 1.5, height + 1.5), (-1.5, height / 2))]
    z = rng.uniform(1.0, 3.0, n - len(pts))
    u, v = rng.uniform(-3, width + 3, z.size), rng.uniform(-3, height + 3, z.size)
    pts += [at_pixel(cam, a, b, c) for a, b, c in zip(u, v, z)]
    order = rng.permutation(n)
    return case(f'scatter_{n}_{width}x{height}_ps{point_size}', np.asarray(pts)[order], cam, width, height, point_size)


def ties_equal():
    cam = ortho(9, 7)
    pts = [at_pixel(cam, 4.5, 3.5, 2.0)] * 64 + [at_pixel(cam, 1.5, 1.5, 1.0)] * 3 + [at_pixel(cam, 4.5, 3.5, 5.0)]
    return case('ties_equal', pts, cam, 9, 7, 1)


def ties_round():
    """the eye 100 behind: zc = z + 100 differs in double between neighbouring float32 z and rounds to one float32.
    The point that is FARTHER in double has the lower index and must win."""
    cam = ortho(8, 6, eye=(0.0, 0.0, -100.0))
    pts = []
    for k, z in enumerate((1.0, 2.5, 7.0)):
        lo, hi = F32(z), np.nextafter(F32(z), F32(100))
        assert F32(np.float64(lo) + 100.0) == F32(np.float64(hi) + 100.0) and np.float64(lo) != np.float64(hi)
        pts += [[k - 3 + 0.5, 0.5, hi], [k - 3 + 0.5, 0.5, lo]]
    return case('ties_round', pts, cam, 8, 6, 0)


def ties_ulp():
    """one float32 ulp apart: the nearer wins, whatever its index"""
    cam = ortho(8, 6)
    pts = []
    for k, z in enumerate((0.5, 2.0, 33.0)):
        near, far = F32(z), np.nextafter(F32(z), F32(100))
        pts += [[k - 3 + 0.5, 0.5, far], [k - 3 + 0.5, 0.5, near]] if k % 2 == 0 else \
            [[k - 3 + 0.5, 0.5, near], [k - 3 + 0.5, 0.5, far]]
    return case('ties_ulp', pts, cam, 8, 6, 0)


def cull_near_far():
    cam = persp(16, 12, near=1.0, far=2.0)
    one, two = F32(1), F32(2)
    zs = [np.nextafter(one, F32(0)), one, np.nextafter(one, two), np.nextafter(two, one), two, np.nextafter(two, F32(3))]
    pts = [at_pixel(cam, 2.5 * k + 1, 6.5, float(z)) for k, z in enumerate(zs)]
    for i in range(len(pts)):
        pts[i][2] = zs[i]                                                    # (the exact float32 depth)
    return case('cull_near_far', pts, cam, 16, 12, 1)


def cull_not_finite():
    cam = persp(16, 12)
    pts = [[0.0, 0.0, 1.5]]
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = [0.1, 0.1, 1.5]
            p[axis] = bad
            pts.append(p)
    pts += [[1e30, 0.0, 1.5], [0.0, -1e30, 1.5], [1e30, 1e30, 1e30], [0.2, 0.1, 1.25]]
    cams = [cam, ortho(16, 12), ortho(16, 12, near=0.0, far=10.0)]
    return case('cull_not_finite', pts, cams, 16, 12, 1)


def cull_overflow():
    """a tiny positive zc with near below it: xc / zc overflows to inf and the window test culls the point"""
    cam = persp(8, 8, near=1e-305, eye=(0.0, 0.0, -1e-300))
    pts = [[3e38, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, -3e38, 0.0], [1e-38, 0.0, 0.0]]
    return case('cull_overflow', pts, cam, 8, 8, 0)


def ortho_negative():
    """negative depths, and -0.0 next to +0.0 (both are stored as +0.0: the lower index wins)"""
    cam = ortho(10, 6)
    pts = [[-3.5, 0.5, -2.0], [-3.5, 0.5, -2.5], [-3.5, 0.5, 1.0],
           [0.5, 0.5, 0.0], [0.5, 0.5, -0.0], [2.5, 0.5, -0.0], [2.5, 0.5, 0.0],
           [4.5, -1.5, -1e-30], [4.5, -1.5, -0.0], [-1.5, -1.5, -np.inf]]
    return case('ortho_negative', pts, cam, 10, 6, 0)


def world_radius(kind):
    """depths that give r = 0, radii in between and r clipped at 16"""
    if kind == 'perspective':
        cam = persp(70, 50, f=32.0)
        spots = [(10.5, 10.5, 40.0), (35.5, 25.5, 0.9), (60.5, 40.5, 1.0), (20.5, 40.5, 4.0), (50.5, 8.5, 3.2),
                 (5.5, 45.5, 15.9), (65.5, 3.5, 16.1), (35.5, 48.5, 2.0)]
        pts = [at_pixel(cam, u, v, z) for u, v, z in spots]
        return case('world_radius_perspective', pts, cam, 70, 50, 0, 0.5)
    pts = [[-2.0, 1.0, 3.0], [2.0, -1.0, 1.0], [0.0, 0.0, 2.0]]
    return [case(f'world_radius_orthographic_{r}', pts, ortho(40, 30, f=f), 40, 30, 0, 0.5)
            for r, f in ((0, 1.5), (5, 11.0), (16, 40.0))]


def three_views(seed=11):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, (300, 3)) * (2.0, 1.5, 0.8)
    lo, hi = pts.min(0), pts.max(0)
    cams = [UR.named_view('iso', lo, hi, (40, 30)), UR.named_view('top', lo, hi, (40, 30), kind='orthographic'),
            UR.named_view('side', lo, hi, (40, 30), fov=70.0)]
    return case('three_views', pts, cams, 40, 30, 1)


def lattice():
    """coordinates at multiples of 0.02 seen straight down with f = 50: u lands exactly on a pixel boundary wherever
    the float32 coordinate is exact (multiples of 0.5) and a hair to either side of one everywhere else"""
    kx, ky = np.arange(-50, 51), np.arange(-6, 7)
    x, y, z = np.meshgrid(kx * 0.02, ky * 0.02, np.array([0.0, 0.02]), indexing='ij')
    pts = np.stack([x, y, z], -1).reshape(-1, 3)
    cam = ortho(104, 26, f=50.0, eye=(0.0, 0.0, 1.0), rot=DOWN)
    return case('lattice', pts, cam, 104, 26, 0)


def tiny(width, height, seed):
    """an image with no side longer than four pixels, every pixel owned, at mixed depths: at radius 4 every
    neighbour of every pixel lies outside the image"""
    rng = np.random.default_rng(seed)
    cam = ortho(width, height)
    pts = [at_pixel(cam, x + 0.5, y + 0.5, z) for y in range(height) for x in range(width)
           for z in rng.uniform(1.0, 3.0, 2)]
    return case(f'tiny_{width}x{height}', pts, cam, width, height, 0)


def raster_cases():
    cam1 = ortho(1, 1)
    cases = [case('empty', np.zeros((0, 3)), persp(5, 4), 5, 4, 1),
             case('one_pixel', [[0.0, 0.0, 1.0]], cam1, 1, 1, 0),
             case('one_pixel_wide', [[0.0, 0.0, 1.0]], cam1, 1, 1, 16)]
    cases += [scatter(1, 257, 33, 17, 0), scatter(2, 1025, 130, 67, 0),
              scatter(3, 257, 33, 17, 2), scatter(4, 1025, 130, 67, 2),
              scatter(5, 257, 33, 17, 16), scatter(6, 257, 130, 67, 16)]
    cases += [ties_equal(), ties_round(), ties_ulp(), cull_near_far(), cull_not_finite(), cull_overflow(),
              ortho_negative(), world_radius('perspective')] + world_radius('orthographic')
    cases += [three_views(), lattice(), tiny(3, 3, 41), tiny(4, 2, 42)]
    return cases


RASTER_CASES = raster_cases()
RASTER = {c['name']: c for c in RASTER_CASES}
assert len(RASTER) == len(RASTER_CASES)

# (raster case, edl = (strength, radius, scale) or None, background)
SHADE_CASES = [('scatter_1025_130x67_ps2', None, (255, 255, 255)),
               ('scatter_1025_130x67_ps2', (0.0, 1, 0.3), (255, 255, 255)),
               ('scatter_1025_130x67_ps2', (1.5, 1, 0.3), (10, 20, 30)),
               ('scatter_1025_130x67_ps2', (1.0, 4, 0.05), (255, 255, 255)),
               ('three_views', (2.0, 2, 0.2), (0, 0, 0)),
               ('one_pixel', (1.0, 1, 1.0), (255, 255, 255)),
               ('ortho_negative', (1.0, 4, 0.5), (1, 2, 3)),
               ('cull_overflow', (3.0, 4, 1e-3), (255, 255, 255)),
               ('world_radius_perspective', (1.0, 1, 0.5), (255, 255, 255)),
               ('tiny_3x3', (1.0, 4, 0.5), (255, 255, 255)),       # every neighbour outside: count == 0 everywhere
               ('tiny_3x3', (1.0, 1, 0.5), (255, 255, 255)),
               ('tiny_4x2', (2.0, 4, 0.5), (0, 0, 0)),
               ('tiny_4x2', (2.0, 1, 0.5), (0, 0, 0))]
SHADE_IDS = [f'{name}-{"flat" if edl is None else "edl_%g_%d_%g" % edl}' for name, edl, _ in SHADE_CASES]


def colors_of(c, seed=99):
    return np.random.default_rng(seed).integers(0, 256, (max(len(c['coords']), 1), 3)).astype(np.uint8)


def raster_args(c):
    return (c['coords'], c['cams'], c['width'], c['height'], c['point_size'], c['world_radius'])
