"""Section 10 on the GPU (include/parallel_ray_tracing.h): photon_tomo_deflect, photon_tomo_deflect_adjoint and
photon_tomo_reconstruct_deflections against the f64 host model of photon_amd/tomography.py on the shared cases of
deflection_cases.py, the adjoint identity on the device, the identity that ties the new operator to photon_tomo_project,
the solver's parity at fixed iteration counts and at convergence, the blob from its views' deflections, and the refusals."""
import ctypes

import numpy as np
import pytest

import deflection_cases as dc
import tomography_cases as tc
from photon_amd import tomography as tm
from photon_amd.library import photon_tomo_stats_t

pytestmark = pytest.mark.gpu

# deflect: the device runs the model's operations in the model's order; deflect_adjoint: only the order of a voxel's sum
# differs.  Both bounds are relative to the largest output, as section 9's are.
OPERATOR_RTOL = 1e-12


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def on_device():
    """Per case: the case, its rays and vectors on the device, a random field and two random ray vectors with the model's
    D f and D^T y."""
    made = {}

    def get(name):
        if name not in made:
            c = dc.CASES[name]()
            rng = np.random.default_rng(17)
            f, y1, y2 = rng.normal(size=c.shape), rng.normal(size=c.n_rays), rng.normal(size=c.n_rays)
            made[name] = dict(case=c, rays=[dev(a) for a in c.rays], f=f, y1=y1, y2=y2,
                              Df=tm.deflect_model(f, c.spacing, c.origin, *c.rays, taps=c.taps),
                              DTy=tm.deflect_adjoint_model(y1, y2, *c.grid, *c.rays, taps=c.taps))
        return made[name]
    return get


def ray_pointers(s):
    return [t.data_ptr() for t in s["rays"]]


def deflect(photon, s, f, stream=None):
    """stream: a torch.cuda.Stream to run on (None = the null stream)."""
    import torch
    c = s["case"]
    g1 = torch.full((c.n_rays,), 7.0, dtype=torch.float64, device="cuda")
    g2 = torch.full((c.n_rays,), 7.0, dtype=torch.float64, device="cuda")
    df = dev(f)
    torch.cuda.synchronize()                                    # the inputs are there before another stream reads them
    photon.tomo_deflect(df.data_ptr(), *c.grid, *ray_pointers(s), c.n_rays, g1.data_ptr(), g2.data_ptr(),
                        stream=0 if stream is None else stream.cuda_stream)
    (torch.cuda if stream is None else stream).synchronize()
    return g1.cpu().numpy(), g2.cpu().numpy()


def deflect_adjoint(photon, s, y1, y2, v0=None, stream=None):
    import torch
    c = s["case"]
    v = torch.zeros(c.shape, dtype=torch.float64, device="cuda") if v0 is None else dev(v0)
    d1, d2 = dev(y1), dev(y2)                                   # both alive until the call has run
    torch.cuda.synchronize()
    photon.tomo_deflect_adjoint(d1.data_ptr(), d2.data_ptr(), *c.grid, *ray_pointers(s), c.n_rays, v.data_ptr(),
                                stream=0 if stream is None else stream.cuda_stream)
    (torch.cuda if stream is None else stream).synchronize()
    return v.cpu().numpy()


@pytest.mark.parametrize("name", list(dc.CASES))
def test_deflect_matches_the_model(photon, on_device, name):
    s = on_device(name)
    got, want = deflect(photon, s, s["f"]), s["Df"]
    size = max(np.abs(want[0]).max(), np.abs(want[1]).max())
    err = max(float(np.abs(g - w).max()) for g, w in zip(got, want)) / size
    print(f"{name}: {s['case'].n_rays} rays, {s['case'].taps.ray.size} taps, max |device - model| / max |g| = {err:.2e}, "
          f"{int((got[0] != want[0]).sum())} and {int((got[1] != want[1]).sum())} rays differ")
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()     # every step is one f64 operation in the model's order
    if name == "random":
        for ray in ("miss_beside", "miss_diagonal", "zero_dir", "nan_origin"):
            assert got[0][tc.edge_ray(ray)] == 0.0 and got[1][tc.edge_ray(ray)] == 0.0, ray
        assert got[0][dc.ZERO_T1] == 0.0 and got[1][dc.ZERO_T1] != 0.0
        assert got[0][dc.NAN_T2] == 0.0 and got[1][dc.NAN_T2] == 0.0
        assert abs(got[0][dc.PARALLEL_T1]) <= OPERATOR_RTOL * size


@pytest.mark.parametrize("name", list(dc.CASES))
def test_deflect_adjoint_matches_the_model(photon, on_device, name):
    s = on_device(name)
    got, want = deflect_adjoint(photon, s, s["y1"], s["y2"]), s["DTy"]
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{name}: max |device - model| / max |v| = {err:.2e}")
    assert err <= OPERATOR_RTOL


def test_deflect_adjoint_adds_into_v(photon, on_device):
    s = on_device("random")
    v0 = np.random.default_rng(6).normal(size=s["case"].shape) * np.abs(s["DTy"]).max()
    got, want = deflect_adjoint(photon, s, s["y1"], s["y2"], v0), v0 + s["DTy"]
    assert np.abs(got - want).max() <= OPERATOR_RTOL * np.abs(want).max()
    assert np.abs(got - s["DTy"]).max() > 0.1 * np.abs(want).max()
    zero = np.zeros(s["case"].n_rays)
    assert (deflect_adjoint(photon, s, zero, zero, v0) == v0).all()      # y1 = y2 = 0 adds nothing


@pytest.mark.parametrize("name", list(dc.CASES))
def test_adjoint_identity_on_the_device(photon, on_device, name):
    s = on_device(name)
    g1, g2 = deflect(photon, s, s["f"])
    lhs = float(np.dot(s["y1"], g1) + np.dot(s["y2"], g2))
    rhs = float(np.dot(deflect_adjoint(photon, s, s["y1"], s["y2"]).ravel(), s["f"].ravel()))
    print(f"{name}: <y, D x> = {lhs:.15e}, <D^T y, x> = {rhs:.15e}, relative difference {abs(lhs - rhs) / abs(lhs):.1e}")
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


@pytest.mark.parametrize("name", ["random", "views"])
def test_central_difference_of_the_device_projector_is_the_operator(photon, on_device, name):
    """photon_tomo_project at origins +- delta tau against photon_tomo_deflect: the rays, delta and bound of the model's test
    (test_tomo_deflection.py)."""
    import torch
    s = on_device(name)
    c = s["case"]
    g = deflect(photon, s, s["f"])
    f, d = dev(s["f"]), s["rays"][1]

    def project(origins):
        o, p = dev(origins), torch.empty((c.n_rays,), dtype=torch.float64, device="cuda")
        photon.tomo_project(f.data_ptr(), *c.grid, o.data_ptr(), d.data_ptr(), c.n_rays, p.data_ptr())
        torch.cuda.synchronize()
        return p.cpu().numpy()

    for j, tau in enumerate((c.t1, c.t2)):
        tau = np.where(np.isfinite(tau), tau, 0.0)
        keep, crossing = dc.same_cells(c, tau)
        diff = (project(dc.shifted_origins(c, tau, 1.0)) - project(dc.shifted_origins(c, tau, -1.0))) / (2.0 * dc.DELTA)
        err = float(np.abs(diff - g[j])[keep].max() / np.abs(g[j]).max())
        print(f"{name}, component {j + 1}: {keep.sum()} of {crossing.sum()} rays kept, max error / max |D f| = {err:.1e}")
        assert keep.sum() >= 0.9 * crossing.sum()
        assert err <= 1e-10


# ---- "runs": the adjoint's lane merge in exact arithmetic ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    """dc.runs_case on the device with the model's D^T y: every sum is exact (test_tomo_deflection.py proves it in rational
    arithmetic), so the device owes the model's bits in whatever order its lanes merge and its atomics land."""
    c = dc.runs_case()
    return dict(case=c, rays=[dev(a) for a in c.rays], DTy=tm.deflect_adjoint_model(c.y1, c.y2, *c.grid, *c.rays, taps=c.taps))


@pytest.fixture(scope="module")
def side_stream():
    import torch
    return torch.cuda.Stream()


def test_runs_deflect_adjoint_is_the_model_bit_for_bit(photon, runs):
    c = runs["case"]
    got = deflect_adjoint(photon, runs, c.y1, c.y2)
    print(f"runs: {int((got != runs['DTy']).sum())} of {got.size} voxels differ, {int((runs['DTy'] != 0).sum())} are not 0")
    assert np.array_equal(got, runs["DTy"])


def test_runs_deflect_adjoint_adds_into_whole_numbers_bit_for_bit(photon, runs):
    c = runs["case"]
    v0 = tc.whole_numbers(np.random.default_rng(6), c.shape, top=100)
    got = deflect_adjoint(photon, runs, c.y1, c.y2, v0)
    assert np.array_equal(got, v0 + runs["DTy"])
    assert not np.array_equal(got, runs["DTy"])


def test_runs_deflect_is_the_model_bit_for_bit(photon, runs):
    c = runs["case"]
    f = np.random.default_rng(17).normal(size=c.shape)
    got, want = deflect(photon, runs, f), tm.deflect_model(f, c.spacing, c.origin, *c.rays, taps=c.taps)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_runs_on_a_side_stream(photon, runs, side_stream):
    """The `stream` argument of photon_tomo_deflect and photon_tomo_deflect_adjoint: the same bits from a stream of the
    caller's."""
    c = runs["case"]
    assert np.array_equal(deflect_adjoint(photon, runs, c.y1, c.y2, stream=side_stream), runs["DTy"])
    f = np.random.default_rng(17).normal(size=c.shape)
    got, want = deflect(photon, runs, f, stream=side_stream), tm.deflect_model(f, c.spacing, c.origin, *c.rays, taps=c.taps)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the solver -------------------------------------------------------------------------------------------------------------
def both(photon, c, g1, g2, **kw):
    want, ws = tm.reconstruct_deflections_model(g1, g2, *c.grid, *c.rays, taps=c.taps, **kw)
    got, gs = photon.tomo_reconstruct_deflections(g1, g2, *c.grid, *c.rays, **kw)
    return got, gs, want, ws


def assert_statistics(gs, ws, residual_rtol=None):
    """The device's stats against the model's: the whole numbers equal, the residual within residual_rtol (None =
    RESIDUAL_RTOL) of the model's."""
    print(f"stats device {gs}, model {ws}")
    for k in ("iterations", "converged", "unknowns", "rays_used"):
        assert gs[k] == ws[k], (k, gs, ws)
    assert abs(gs["residual"] - ws["residual"]) <= (RESIDUAL_RTOL if residual_rtol is None else residual_rtol) * ws["residual"], (gs, ws)


# CG amplifies the adjoint's summation-order noise, and the deflection problem is worse conditioned than section 9's: with the
# model's tap order permuted in the adjoint the "random" solutions spread by 7.6e-15 of max |f| after 8 iterations at lambda
# 0.05 (3.9e-8 after 20), and by 2.8e-12 after 20 iterations at lambda 50 (1.5e-15 after 8).  (a) keeps 130 x the first
# spread, (b) 350 x the second.  The counts (c) to (g) are there for the statistics, as section 9's are: odd and even, at a
# check, between checks and none; the model's residuals after 0, 1, 7, 8, 9 and 17 iterations at lambda 50 are 1, 0.4645,
# 0.02681, 0.01899, 0.01341 and 7.07e-4, and under a permuted tap order they moved by at most 1.5e-15 of themselves (20
# iterations; lambda 0.05, 8 iterations: 9.4e-16): RESIDUAL_RTOL keeps 650 x.  The solutions moved by at most 1.6e-15 of max
# |f| up to 9 iterations and by 3.4e-13 after 17: (g) keeps 300 x.
RESIDUAL_RTOL = 1e-12


@pytest.mark.parametrize("label,lam,iterations,rtol", [("a", 0.05, 8, 1e-12), ("b", 50.0, 20, 1e-9), ("c", 50.0, 0, 1e-12),
                                                       ("d", 50.0, 1, 1e-12), ("e", 50.0, 7, 1e-12), ("f", 50.0, 9, 1e-12),
                                                       ("g", 50.0, 17, 1e-10)])
def test_fixed_iteration_parity(photon, label, lam, iterations, rtol):
    c = dc.random_case()
    g1, g2, w, support = dc.random_problem(c)
    got, gs, want, ws = both(photon, c, g1, g2, w=w, support=support, lam=lam, tol=0.0, max_iter=iterations)
    err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    print(f"({label}) lambda {lam}, {iterations} iterations: max |device - model| / max |f| = {err:.2e}; residual device "
          f"{gs['residual']:.3e}, model {ws['residual']:.3e}")
    assert_statistics(gs, ws)
    assert gs["iterations"] == iterations and gs["unknowns"] == int(support.sum()) and gs["converged"] == 0
    assert (got[support == 0] == 0).all()
    assert err <= rtol
    if iterations == 0:
        assert (got == 0).all() and gs["residual"] == 1.0


def test_fixed_iteration_parity_with_dense_rays(photon):
    """The solver where the adjoint merges lanes.  With the model's tap order permuted the "dense" solution moved by 1.9e-15 of
    max |f| after 8 iterations at lambda 50 (2.5e-15 at lambda 1): the operators' bound keeps 500 x; its residual moved by
    6.8e-16 of itself."""
    c = dc.dense_case()
    g1, g2 = dc.blob_deflections(c)
    support = tc.sphere_support(c.case)
    got, gs, want, ws = both(photon, c, g1, g2, w=tc.ray_weights(c.n_rays), support=support, lam=50.0, tol=0.0, max_iter=8)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"dense, lambda 50, 8 iterations: max |device - model| / max |f| = {err:.2e}")
    assert_statistics(gs, ws)
    assert (got[support == 0] == 0).all()
    assert err <= OPERATOR_RTOL


# The dense rays on 2^3, 3^3 and 4^3: every voxel and 2 iterations, as in section 9's test of the same name.  With the model's
# tap order permuted (8 permutations) the solution after 2 iterations moved by at most 1.9e-14 of max |f| and the residual by
# 8.3e-14 of itself: both bounds keep 120 x.
COARSE_RTOL = 1e-11


@pytest.mark.parametrize("name", ["coarse2", "coarse3", "coarse4"])
def test_fixed_iteration_parity_with_whole_waves_in_one_voxel(photon, name):
    c = dc.CASES[name]()
    g1, g2 = dc.blob_deflections(c)
    got, gs, want, ws = both(photon, c, g1, g2, w=tc.ray_weights(c.n_rays), lam=50.0, tol=0.0, max_iter=2)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{name}, lambda 50, 2 iterations: max |device - model| / max |f| = {err:.2e}")
    assert_statistics(gs, ws, COARSE_RTOL)
    assert gs["iterations"] == 2 and gs["unknowns"] == c.taps.n_voxels
    assert err <= COARSE_RTOL


# ---- the capped grid: more voxels than kMaxBlocks * kThreads = 262 144 (section 9's test of the same name) -----------------------
# With the model's tap order permuted the solutions moved by at most 7.5e-16 of max |f| and the residuals by 1.7e-16; on every
# voxel, where the second trip of the element-wise kernels counts (the solution there reaches 0.41 of max |f|), by 1.1e-15 and
# 6.2e-16.
@pytest.mark.parametrize("n,iterations,sphere", [(65, 3, True), (64, 2, True), (65, 3, False)], ids=["65-sphere", "64-sphere", "65-every-voxel"])
def test_fixed_iteration_parity_on_a_capped_grid(photon, n, iterations, sphere):
    c = dc.view_frames_of(tc.view_case(n, 24, 4), k_views=4)
    g1, g2 = dc.blob_deflections(c)
    support = tc.sphere_support(c.case) if sphere else np.ones(c.shape, np.uint8)
    got, gs, want, ws = both(photon, c, g1, g2, w=tc.ray_weights(c.n_rays), support=support, lam=50.0, tol=0.0, max_iter=iterations)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{n}^3, {'sphere' if sphere else 'every voxel'}, lambda 50, {iterations} iterations: max |device - model| / max |f| = {err:.2e}")
    assert_statistics(gs, ws)
    assert gs["iterations"] == iterations and gs["unknowns"] == int(support.sum()) and gs["converged"] == 0
    assert (got[support == 0] == 0).all()
    assert err <= OPERATOR_RTOL


# ---- where the solver stops, and what it reports then ------------------------------------------------------------------------
@pytest.mark.parametrize("stop,before", [(8, 7), (16, 8)])
def test_tolerance_stops_at_a_check_before_the_limit(photon, stop, before):
    """tol between the model's residuals after `before` and after `stop` iterations (their geometric mean), max_iter = stop +
    1: the check after `stop` iterations ends the run, one iteration before the limit would (section 9's test of the same
    name).  After 16 iterations the solution moves by 1.5e-13 of max |f| under a permuted tap order: the bound of (g)."""
    c = dc.random_case()
    g1, g2, w, support = dc.random_problem(c)
    kw = dict(w=w, support=support, lam=50.0)
    r = [tm.reconstruct_deflections_model(g1, g2, *c.grid, *c.rays, taps=c.taps, tol=0.0, max_iter=k, **kw)[1]["residual"]
         for k in (before, stop)]
    tol = float(np.sqrt(r[0] * r[1]))
    assert r[1] < tol < r[0]
    got, gs, want, ws = both(photon, c, g1, g2, tol=tol, max_iter=stop + 1, **kw)
    assert_statistics(gs, ws)
    assert gs["iterations"] == stop and gs["converged"] == 1
    assert np.abs(got - want).max() <= (OPERATOR_RTOL if stop == 8 else 1e-10) * np.abs(want).max()


def test_an_empty_support_needs_no_iteration(photon):
    c = dc.random_case()
    g1, g2, w, _ = dc.random_problem(c)
    got, gs, want, ws = both(photon, c, g1, g2, w=w, support=np.zeros(c.shape, np.uint8), lam=50.0, tol=0.0, max_iter=9)
    assert_statistics(gs, ws)
    assert gs["iterations"] == 0 and gs["unknowns"] == 0 and gs["converged"] == 1 and gs["residual"] == 0.0
    assert (got == 0).all() and (want == 0).all()


def test_pointer_form_on_a_side_stream(photon, side_stream):
    """tomo_reconstruct_deflections_ptr on device tensors and a stream of the caller's against the array form and the model."""
    import torch
    c = dc.random_case()
    g1, g2, w, support = dc.random_problem(c)
    kw = dict(lam=50.0, tol=0.0, max_iter=9)
    _, array_stats, want, ws = both(photon, c, g1, g2, w=w, support=support, **kw)
    d1, d2, dw, ds = dev(g1), dev(g2), dev(w), dev(support)
    rays = [dev(a) for a in c.rays]
    f = torch.full(c.shape, 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gs = photon.tomo_reconstruct_deflections_ptr(d1.data_ptr(), d2.data_ptr(), *c.grid, *(t.data_ptr() for t in rays), c.n_rays,
                                                 f.data_ptr(), d_w_ptr=dw.data_ptr(), d_support_ptr=ds.data_ptr(),
                                                 stream=side_stream.cuda_stream, **kw)
    got = f.cpu().numpy()                                       # the call has synchronised its stream
    for k in ("iterations", "converged", "unknowns", "rays_used"):
        assert gs[k] == array_stats[k], (k, gs, array_stats)
    assert_statistics(gs, ws)
    assert (got[support == 0] == 0).all()
    assert np.abs(got - want).max() <= OPERATOR_RTOL * np.abs(want).max()


def test_converged_parity(photon):
    """lambda 5, tol 1e-10: the model converges in 136 iterations; with its tap order permuted the solution moved by 5.3e-11 of
    max |f|.  The bound keeps 1900 x."""
    c = dc.random_case()
    g1, g2, w, support = dc.random_problem(c)
    got, gs, want, ws = both(photon, c, g1, g2, w=w, support=support, lam=5.0, tol=1e-10, max_iter=2000)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"(c) lambda 5, tol 1e-10: device {gs['iterations']} iterations, model {ws['iterations']}; max |device - model| / max |f| = "
          f"{err:.2e}")
    assert gs["converged"] == 1 and ws["converged"] == 1
    assert abs(gs["iterations"] - ws["iterations"]) <= tm.CHECK_EVERY
    assert gs["unknowns"] == ws["unknowns"] and gs["rays_used"] == ws["rays_used"]
    assert err <= 1e-7


def test_views_reconstruct_the_blob(photon):
    c = dc.views_case()
    truth, (g1, g2), support = tc.blob_field(c.case), dc.blob_deflections(c), tc.sphere_support(c.case)
    f, st = photon.tomo_reconstruct_deflections(g1, g2, *c.grid, *c.rays, support=support, lam=1.0, tol=0.0, max_iter=50)
    err = tc.rel_l2(f, truth)
    print(f"views' deflections on the device: relative L2 error inside the sphere {err:.4f} (model 0.0553, bound 0.07)")
    assert st["iterations"] == 50 and st["unknowns"] == int(support.sum()) and st["rays_used"] == c.n_rays
    assert (f[support == 0] == 0).all()
    assert err <= 0.07


def test_zero_data_needs_no_iteration(photon):
    c = dc.random_case()
    zero = np.zeros(c.n_rays)
    f, st = photon.tomo_reconstruct_deflections(zero, zero, *c.grid, *c.rays)
    assert st["iterations"] == 0 and st["converged"] == 1 and st["residual"] == 0.0 and (f == 0).all()


def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    n = 8
    rays = torch.ones((n, 3), dtype=torch.float64, device="cuda")
    vals = torch.zeros((n,), dtype=torch.float64, device="cuda")
    out = torch.full((4, 4, 4), 7.0, dtype=torch.float64, device="cuda")
    outp = torch.full((2, n), 7.0, dtype=torch.float64, device="cuda")
    r, v, o = (ctypes.c_void_p(t.data_ptr()) for t in (rays, vals, out))
    op1, op2 = ctypes.c_void_p(outp[0].data_ptr()), ctypes.c_void_p(outp[1].data_ptr())
    nan, inf = float("nan"), float("inf")
    arr = lambda *x: (ctypes.c_double * 3)(*x)      # noqa: E731
    sp, og = arr(1.0, 1.0, 1.0), arr(0.0, 0.0, 0.0)
    good = dict(nx=4, ny=4, nz=4, sp=sp, og=og, o=r, d=r, t1=r, t2=r, n=n)
    grid_cases = [("nx 1", dict(nx=1)), ("ny 1", dict(ny=1)), ("nz 1", dict(nz=1)), ("too many voxels", dict(nx=2048, ny=2048, nz=2048)),
                  ("no rays", dict(n=0)), ("spacing 0", dict(sp=arr(1.0, 0.0, 1.0))), ("spacing < 0", dict(sp=arr(-1.0, 1.0, 1.0))),
                  ("spacing nan", dict(sp=arr(1.0, 1.0, nan))), ("spacing inf", dict(sp=arr(inf, 1.0, 1.0))),
                  ("origin nan", dict(og=arr(0.0, nan, 0.0))), ("origin inf", dict(og=arr(0.0, 0.0, inf))),
                  ("null spacing", dict(sp=None)), ("null origin", dict(og=None)),
                  ("null origins", dict(o=None)), ("null dirs", dict(d=None)), ("null t1", dict(t1=None)), ("null t2", dict(t2=None))]

    def grid_args(g):
        return (g["nx"], g["ny"], g["nz"], g["sp"], g["og"], g["o"], g["d"], g["t1"], g["t2"], g["n"])

    def check(name, what, rc, st=None):
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc == 1, (name, what)
        assert len(err.strip().splitlines()) == 1 and f"photon: {name}:" in err, (name, what, err)
        assert (out == 7.0).all().item() and (outp == 7.0).all().item(), (name, what)
        if st is not None:
            assert list(st.as_dict().values()) == [-5, -5, -5, -5, -5.0], (name, what)

    capfd.readouterr()
    for what, change in grid_cases:
        g = {**good, **change}
        check("photon_tomo_deflect", what, L.photon_tomo_deflect(o, *grid_args(g), op1, op2, None))
        check("photon_tomo_deflect_adjoint", what, L.photon_tomo_deflect_adjoint(v, v, *grid_args(g), o, None))
    check("photon_tomo_deflect", "null d_f", L.photon_tomo_deflect(None, *grid_args(good), op1, op2, None))
    check("photon_tomo_deflect", "null d_g1", L.photon_tomo_deflect(o, *grid_args(good), None, op2, None))
    check("photon_tomo_deflect", "null d_g2", L.photon_tomo_deflect(o, *grid_args(good), op1, None, None))
    check("photon_tomo_deflect_adjoint", "null d_y1", L.photon_tomo_deflect_adjoint(None, v, *grid_args(good), o, None))
    check("photon_tomo_deflect_adjoint", "null d_y2", L.photon_tomo_deflect_adjoint(v, None, *grid_args(good), o, None))
    check("photon_tomo_deflect_adjoint", "null d_v", L.photon_tomo_deflect_adjoint(v, v, *grid_args(good), None, None))
    solver_cases = grid_cases + [("lambda < 0", dict(lam=-1.0)), ("lambda nan", dict(lam=nan)), ("tol < 0", dict(tol=-1.0)),
                                 ("tol nan", dict(tol=nan)), ("max_iter < 0", dict(it=-1)), ("null g1", dict(g1=None)),
                                 ("null g2", dict(g2=None)), ("null f", dict(f=None))]
    for what, change in solver_cases:
        g = {**good, **dict(lam=1.0, tol=1e-6, it=10, g1=v, g2=v, f=o), **change}
        st = photon_tomo_stats_t(-5, -5, -5, -5, -5.0)
        rc = L.photon_tomo_reconstruct_deflections(g["g1"], g["g2"], None, None, *grid_args(g), g["lam"], g["tol"], g["it"], g["f"],
                                                   ctypes.byref(st), None)
        check("photon_tomo_reconstruct_deflections", what, rc, st)
    c = dc.random_case()                                                              # accepted calls are silent
    f, st = photon.tomo_reconstruct_deflections(np.ones(c.n_rays), np.ones(c.n_rays), *c.grid, *c.rays, max_iter=3)
    assert capfd.readouterr().err == "" and st["iterations"] == 3
