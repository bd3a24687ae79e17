"""Inputs and host models for tests/test_generators.py (CPU) and tests/test_generators_gpu.py: the kernels that MAKE the
inputs -- the Gaussian volume, the PIV sources and their extent, the advected frame 2 -- and the one that makes the final
picture, photon_postprocess_u16, on inputs with no symmetry to hide behind: three different sides, spacings, origins and
centres; a velocity grid with nx != ny != nz that the particles leave through every face; boxes with lo != -hi; images
with odd sides, every pixel class and exact rounding ties."""
import math

import numpy as np

from photon_amd import piv_pairs as pp
from photon_amd import scenes
from photon_amd.ray_tracing import single_lens_camera

# ---- 1. Gaussian volume -----------------------------------------------------------------------------------------------
RHO0, AMP = 1.225, 0.2
_SPACING = (310.0, 295.5, 402.25)
_ORIGIN = (-1130.0, 870.0, 300250.0)                 # off the axis in x and y; z where the BOS volumes sit
_CENTRE_AT = (0.3, 0.6, 0.45)                        # of the extent per axis: 1.8, 6.6 and 3.6 spacings in: on no node


def _gauss_case(n):
    extent = [(n[a] - 1) * _SPACING[a] for a in range(3)]
    return dict(n=tuple(n), spacing=_SPACING, origin=_ORIGIN, rho0=RHO0, amp=AMP,
                centre=tuple(_ORIGIN[a] + _CENTRE_AT[a] * extent[a] for a in range(3)), sigma=0.25 * min(extent))


# (nx, ny, nz): three different sides, 756 voxels = two full blocks of 256 and a partial one; and the smallest sides the ABI takes
GAUSS_CASES = {"7x12x9": _gauss_case((7, 12, 9)), "3x3x5": _gauss_case((3, 3, 5))}


def gauss_args(case):
    """The tuple photon.volume_gaussian, photon.density_gaussian_write_nrrd and oracle.volume_gaussian take after their
    first argument(s)."""
    return (case["n"], case["spacing"], case["origin"], case["rho0"], case["amp"], case["centre"], case["sigma"])


def gauss_rho(case):
    """rho0 + amp exp(-|r - centre|^2 / (2 sigma^2)) on the nodes origin + (i, j, k) spacing, f32 [nz][ny][nx]: the
    header's formula (include/parallel_ray_tracing.h, photon_volume_gaussian) with its per-axis spacing, origin and centre,
    one exp of the whole exponent in f64 (the device multiplies three axis profiles: the last ulp of exp apart)."""
    nx, ny, nz = case["n"]
    ax = [case["origin"][a] + case["spacing"][a] * np.arange(m, dtype=np.float64) - case["centre"][a]
          for a, m in enumerate((nx, ny, nz))]
    r2 = ax[2][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[0][None, None, :] ** 2
    return (case["rho0"] + case["amp"] * np.exp(-r2 / (2.0 * case["sigma"] ** 2))).astype(np.float32)


def axis_permutations(rho):
    """The five non-trivial axis permutations of rho, each resampled (nearest node) to rho's own shape where the shapes
    differ: {axes: array}.  What a kernel that mixes up i / j / k, nx / ny / nz or an axis's spacing, origin or centre
    would produce is one of these, or nearer to one of these than to rho."""
    out = {}
    for axes in ((0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        p = np.transpose(rho, axes)
        idx = [np.rint(np.linspace(0, p.shape[a] - 1, rho.shape[a])).astype(int) for a in range(3)]
        out[axes] = p[np.ix_(*idx)]
    return out


# ---- 2. flow sampler --------------------------------------------------------------------------------------------------
BOX_LO, BOX_HI = (-3.0e4, -3.0e4, -7.5e3), (3.0e4, 3.0e4, 7.5e3)                # the usual box of the PIV tests
GRID_LO, GRID_HI = (-1.0e4, -2.0e4, -2.0e3), (2.0e4, 1.0e4, 5.0e3)              # inside it, off its centre on every axis
Z_OBJ = 823668.35
CDF = np.cumsum(np.full(27, 1.0 / 27.0))
FLOW_SEED, FLOW_N, FLOW_T, FLOW_STEPS = 11, 4096, 1.5, 4
SHEET = (730.0, 500.0)                                                           # beam_fwhm, irradiance_constant
NAN_NODE = (1, 2, 3)                                                             # (k, j, i): interior of the (3, 5, 7) grid


def noise_flow(shape=(3, 5, 7), nan_node=None, seed=FLOW_SEED):
    """(u, v, w, spacing, origin) on [GRID_LO, GRID_HI] with shape = (nz, ny, nx) nodes: u, v, w independent uniform noise
    in +-4e3 (f32), so no two nodes, rows or slabs agree and every clamp changes the sample; nan_node: that node's u = NaN."""
    nz, ny, nx = shape
    _, _, _, spacing, origin = pp.grid_nodes(GRID_LO, GRID_HI, (nx, ny, nz))
    rng = np.random.default_rng(seed)
    u, v, w = (rng.uniform(-4.0e3, 4.0e3, shape).astype(np.float32) for _ in range(3))
    if nan_node is not None:
        u[nan_node] = np.nan
    return u, v, w, spacing, origin


def flow_advect(flow, cdf=None, n=FLOW_N, **variant):
    """The host model of the flow cases' frame 2 (pp.advect; with `variant`, advect_variant)."""
    f = advect_variant if variant else pp.advect
    return f(FLOW_SEED, n, BOX_LO, BOX_HI, Z_OBJ, *SHEET, cdf, flow=flow, t=FLOW_T, steps=FLOW_STEPS, **variant)


def beyond_faces(world, lo=GRID_LO, hi=GRID_HI):
    """Share of the points [n][3] beyond each of the grid's six faces: {"x-": ..., "x+": ..., ...}."""
    out = {}
    for a, name in enumerate("xyz"):
        out[name + "-"] = float((world[:, a] < lo[a]).mean())
        out[name + "+"] = float((world[:, a] > hi[a]).mean())
    return out


class _WrongGrid(pp._Grid):
    """pp._Grid with one of the mistakes the asymmetric grid is there to catch."""

    def __init__(self, flow, clamp_weight=True, y_stride_is_ny=False):
        super().__init__(flow)
        self.clamp_weight, self.y_stride_is_ny = clamp_weight, y_stride_is_ny

    def _axis(self, p, a, n):
        f = (p - self.origin[a]) / self.spacing[a]
        c = np.floor(f)
        c = np.where(c >= 0.0, c, 0.0)
        c = np.where(c <= float(n - 2), c, float(n - 2))
        t = f - c
        if self.clamp_weight:
            t = np.where(t > 0.0, t, 0.0)
            t = np.where(t < 1.0, t, 1.0)
        return c.astype(np.int64), t

    def sample(self, x, y, z):
        i, tx = self._axis(x, 0, self.nx)
        j, ty = self._axis(y, 1, self.ny)
        k, tz = self._axis(z, 2, self.nz)
        sy, sz = (self.ny if self.y_stride_is_ny else self.nx), self.nx * self.ny
        b = k * sz + j * sy + i
        g = self.uvw
        tx, ty, tz = tx[:, None], ty[:, None], tz[:, None]
        c0 = pp._lerp(pp._lerp(g[b], g[b + 1], tx), pp._lerp(g[b + sy], g[b + sy + 1], tx), ty)
        c1 = pp._lerp(pp._lerp(g[b + sz], g[b + sz + 1], tx), pp._lerp(g[b + sz + sy], g[b + sz + sy + 1], tx), ty)
        return pp._lerp(c0, c1, tz)


def advect_variant(seed, n, box_min, box_max, z_object, beam_fwhm, irradiance_constant, diameter_cdf=None, flow=None, t=0.0,
                   steps=16, **wrong):
    """pp.advect through a _WrongGrid (clamp_weight=False: extrapolates outside the grid instead of holding the boundary
    value; y_stride_is_ny=True: a row is ny nodes long).  With no mistake asked for it is pp.advect, which the CPU tier
    asserts bit for bit."""
    X, Y, Z, ud = pp._draw(seed, n, box_min, box_max)
    g = _WrongGrid(flow, **wrong)
    h = float(t) / int(steps)
    hh, h6 = 0.5 * h, h / 6.0
    for _ in range(int(steps)):
        k1 = g.sample(X, Y, Z)
        k2 = g.sample(X + hh * k1[:, 0], Y + hh * k1[:, 1], Z + hh * k1[:, 2])
        k3 = g.sample(X + hh * k2[:, 0], Y + hh * k2[:, 1], Z + hh * k2[:, 2])
        k4 = g.sample(X + h * k3[:, 0], Y + h * k3[:, 1], Z + h * k3[:, 2])
        d = k1 + 2.0 * k2 + 2.0 * k3 + k4
        X, Y, Z = X + h6 * d[:, 0], Y + h6 * d[:, 1], Z + h6 * d[:, 2]
    return pp._store(X, Y, Z, ud, z_object, beam_fwhm, irradiance_constant, diameter_cdf)


# ---- 3. extents of generated sources ----------------------------------------------------------------------------------
GEOM = single_lens_camera(lens_model="general", **scenes.SAMPLE_LENS)            # the camera of scenes.piv_scene
EXTENT_N, EXTENT_SEED = 300, 77
_FAR, _NEAR, _THIN, _SHEET_Z = 2.0e5, 2.0e4, 5.0e3, 1.0e3
# name -> (box_min, box_max, near-side box_min, near-side box_max, the long axis): the box reaches 2e5 um from the axis on ONE
# side of one axis only, so max(|box_min|, |box_max|) matters and which of the two is larger changes from case to case
EXTENT_BOXES = {
    "x_low": ((-_FAR, -_THIN, -_SHEET_Z), (_NEAR, _THIN, _SHEET_Z), (-_NEAR, -_THIN, -_SHEET_Z), (_NEAR, _THIN, _SHEET_Z), 0),
    "x_high": ((-_NEAR, -_THIN, -_SHEET_Z), (_FAR, _THIN, _SHEET_Z), (-_NEAR, -_THIN, -_SHEET_Z), (_NEAR, _THIN, _SHEET_Z), 0),
    "y_low": ((-_THIN, -_FAR, -_SHEET_Z), (_THIN, _NEAR, _SHEET_Z), (-_THIN, -_NEAR, -_SHEET_Z), (_THIN, _NEAR, _SHEET_Z), 1),
    "y_high": ((-_THIN, -_NEAR, -_SHEET_Z), (_THIN, _FAR, _SHEET_Z), (-_THIN, -_NEAR, -_SHEET_Z), (_THIN, _NEAR, _SHEET_Z), 1),
}


def extent_call():
    """The scene of test_extent_follows_the_particles_out_of_the_box (tests/test_piv_pairs_gpu.py): scales at which the
    lens-sample cull bites."""
    return scenes.piv_scene(n_particles=EXTENT_N, rays_per_source=1000, mie=True, polydisperse=True, seed=3)


# ---- 4. post-processing -----------------------------------------------------------------------------------------------
POST_SMALL, POST_LARGE = (37, 53), (725, 725)        # (rows, cols); 725^2 > 2048 blocks x 256 threads: the grid-stride loop
POST_DEPTHS, POST_GAINS = (1, 8, 10, 12, 16), (-6.0, 0.0, 25.0)
# 100 * image_noise is then 6.25 exactly, in f32 and in f64: the expected noisy pixel is raw + n0 * 6.25 with no rounding of
# the standard deviation to argue about
POST_NOISE = 0.0625
PHOTON_STREAM_IMAGE_NOISE = 4                        # include/photon_philox.h


def post_image(shape, seed=5):
    """f32 [rows][cols]: positive values over six decades (1e-2 .. 1e4), about 5 % negative, one NaN, one +inf, one -inf,
    and the brightest finite pixel (3e4) in the middle of the array, neither first nor last."""
    rng = np.random.default_rng(seed)
    img = (10.0 ** rng.uniform(-2.0, 4.0, shape)).astype(np.float32)
    neg = rng.random(shape) < 0.05
    img[neg] = -img[neg]
    flat = img.reshape(-1)
    n = flat.size
    flat[n // 2 + 3] = 3.0e4
    flat[7], flat[n // 3], flat[n - 5] = np.nan, np.inf, -np.inf
    return img


def post_finite(img):
    """img with its three non-finite pixels replaced by finite values (for intensity_rescaling off, where the conversion
    of a non-finite float to uint16 is undefined in C and in numpy alike and the header promises nothing)."""
    out = img.copy()
    out[np.isnan(out)] = 12.5
    out[np.isposinf(out)] = 777.75
    out[np.isneginf(out)] = -3.0
    return out


def tie_image(shape=POST_SMALL):
    """Gain 0 dB, depth 8, brightest pixel exactly 255: (255 v) / 255 == v in f32 for v = k + 0.5, k < 255 (255 k + 127.5 has
    17 significant bits), so these pixels are exact ties, even and odd k alike.  Returns (image, flat index of the ties, k)."""
    rng = np.random.default_rng(9)
    img = rng.uniform(0.0, 250.0, shape).astype(np.float32)
    flat = img.reshape(-1)
    k = np.arange(0, 255)
    at = 20 + 3 * k                                   # scattered through the image
    flat[at] = (k + 0.5).astype(np.float32)
    flat[flat.size // 2] = 255.0
    assert flat.size // 2 not in at and at.max() < flat.size
    return img, at, k


def dark_image(shape=POST_SMALL):
    """No positive pixel: zeros (both signs) and negatives -- the max == 0 branch."""
    rng = np.random.default_rng(10)
    img = np.where(rng.random(shape) < 0.5, 0.0, -rng.uniform(0.0, 50.0, shape)).astype(np.float32)
    img.reshape(-1)[::7] = -0.0
    return img


def wrap_image(shape=POST_SMALL):
    """Values in (65535, 2^31) for intensity_rescaling off, log-uniform, plus the two ends next to the limits."""
    rng = np.random.default_rng(12)
    img = (2.0 ** rng.uniform(16.0, 31.0, shape)).astype(np.float32)
    flat = img.reshape(-1)
    flat[0], flat[1], flat[2] = 65536.0, np.nextafter(np.float32(2.0 ** 31), np.float32(0)), 65535.5
    assert (flat > 65535.0).all() and (flat < 2.0 ** 31).all()
    return img


def wrapped_u16(img):
    """What the kernel's comment promises beyond the u16 range: truncation to int64, then the low 16 bits -- written out,
    because numpy's own float -> uint16 cast is C's, undefined out of range."""
    return (np.trunc(np.asarray(img, np.float64)).astype(np.int64) & 0xFFFF).astype(np.uint16)


def crop_requests(rows, cols):
    """(legal, refused) crop requests for a rows x cols image.  A request (r, c) gives 2 (r // 2) - 1 rows from row
    rows // 2 - r // 2: legal while 1 <= r // 2 <= rows // 2 (the same along the columns)."""
    rmax, cmax = 2 * (rows // 2) + 1, 2 * (cols // 2) + 1              # the largest requests that still fit
    legal = [(2, 2), (3, 3), (2, cmax), (rmax, 2), (7, 11), (12, 5), (rows, cols), (rmax, cmax), (rmax - 1, cmax - 1)]
    refused = [(rmax + 1, 2), (2, cmax + 1), (rmax + 1, cmax + 1), (1, 2), (2, 1), (1, 1)]
    return legal, refused


def noise_expectation(raw, n0, image_noise=POST_NOISE):
    """(exact, tol): raw + n0 (100 image_noise) per pixel in f64 -- exact, the product of a 24-bit and a 4-bit significand
    and one sum well inside 53 bits -- and how far an f32 evaluation may be from it.  Unfused, fl(fl(n0 s) + raw): the
    product is off by at most half an f32 ulp of the product and the sum rounds once more, half an f32 ulp of the sum; fused,
    fl(n0 s + raw), only the latter.  So |device - exact| <= ulp32(|n0 s|) / 2 + ulp32(|exact|) / 2 covers both, and nothing
    else does (np.spacing of the value rounded to f32 is the ulp of its binade, or of the next one up at a power of two)."""
    s = 100.0 * float(image_noise)
    assert np.float32(s) == s and np.float32(image_noise) * np.float32(100.0) == np.float32(s)
    prod = np.asarray(n0, np.float64).reshape(np.shape(raw)) * s
    with np.errstate(invalid="ignore"):
        exact = np.asarray(raw, np.float64) + prod
        tol = 0.5 * np.spacing(np.abs(prod).astype(np.float32)).astype(np.float64) + \
            0.5 * np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    return exact, tol


# ---- 5. gzip payloads that lie ----------------------------------------------------------------------------------------
def lying_gzip_payloads(little: bytes):
    """Four compressed payloads for a volume whose raw bytes are `little`, each of which inflates to at least the sizes'
    worth of the right bytes and is still not the file it claims to be: {name: payload}."""
    import gzip
    gz = gzip.compress(little)
    crc = bytearray(gz)
    crc[-8] ^= 0x01                                   # the trailer: CRC32 (4 bytes, little endian), ISIZE (4 bytes)
    isize = bytearray(gz)
    isize[-4:] = (len(little) + 4).to_bytes(4, "little")
    return {"crc_flipped": bytes(crc), "isize_changed": bytes(isize), "inflates_beyond_sizes": gzip.compress(little + b"\x07" * 400),
            "junk_after_the_stream": gz + bytes(range(1, 17))}
