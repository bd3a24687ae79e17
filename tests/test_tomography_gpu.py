"""Section 9 on the GPU (include/parallel_ray_tracing.h): photon_tomo_project, photon_tomo_backproject and
photon_tomo_reconstruct against the f64 host model of photon_amd/tomography.py on the shared cases of tomography_cases.py,
the adjoint identity on the device, the solver's parity at fixed iteration counts and at convergence, the blob
reconstructed from its views, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest

import tomography_cases as tc
from photon_amd import tomography as tm
from photon_amd.library import photon_tomo_stats_t

pytestmark = pytest.mark.gpu

# project: the device runs the model's operations in the model's order; backproject: only the order of a voxel's sum
# differs (a permuted order moved the model by 4e-16 of max |v|).  Both bounds are relative to the largest output.
OPERATOR_RTOL = 1e-12

# The residual of a solve against the model's, relative.  With the model's tap order permuted its residual moved by at most
# 1.8e-15 ("random", lambda 50, 0 to 40 iterations: 40 was the largest; lambda 0.5, 8 iterations: 7.6e-16), 6.5e-15 ("dense",
# 8 iterations) and 8.6e-16 (65^3 and 64^3, 3 and 2 iterations): the bound keeps 150 x the largest of them.
RESIDUAL_RTOL = 1e-12

# "dense": four rays per voxel and axis, runs of up to six adjacent lanes in one voxel; "coarse2" .. "coarse4": the same rays
# on 2^3, 3^3 and 4^3, runs of up to 64, 52 and 34 lanes with ordinary weights (test_tomography.py holds the run lengths); the
# other cases stop at two.  The merge's lane layouts one by one are the "runs" family below.
CASES = {"random": tc.random_case, "views": tc.views_case, "large": tc.large_case, "dense": tc.dense_case,
         "coarse2": functools.partial(tc.coarse_case, 2), "coarse3": functools.partial(tc.coarse_case, 3),
         "coarse4": functools.partial(tc.coarse_case, 4)}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def on_device():
    """Per case: the case, its rays on the device, a random field and a random ray vector with the model's A f and A^T y."""
    made = {}

    def get(name):
        if name not in made:
            c = CASES[name]()
            rng = np.random.default_rng(17)
            f, y = rng.normal(size=c.shape), rng.normal(size=c.n_rays)
            made[name] = dict(case=c, o=dev(c.origins), d=dev(c.dirs), f=f, y=y,
                              Af=tm.project_model(f, c.spacing, c.origin, c.origins, c.dirs, taps=c.taps),
                              ATy=tm.backproject_model(y, *c.grid, c.origins, c.dirs, taps=c.taps))
        return made[name]
    return get


def project(photon, s, f, stream=None):
    """stream: a torch.cuda.Stream to run on (None = the null stream)."""
    import torch
    c = s["case"]
    p = torch.full((c.n_rays,), 7.0, dtype=torch.float64, device="cuda")
    df = dev(f)
    torch.cuda.synchronize()                                    # the inputs are there before another stream reads them
    photon.tomo_project(df.data_ptr(), *c.grid, s["o"].data_ptr(), s["d"].data_ptr(), c.n_rays, p.data_ptr(),
                        stream=0 if stream is None else stream.cuda_stream)
    (torch.cuda if stream is None else stream).synchronize()
    return p.cpu().numpy()


def backproject(photon, s, y, v0=None, stream=None):
    import torch
    c = s["case"]
    v = torch.zeros(c.shape, dtype=torch.float64, device="cuda") if v0 is None else dev(v0)
    dy = dev(y)
    torch.cuda.synchronize()
    photon.tomo_backproject(dy.data_ptr(), *c.grid, s["o"].data_ptr(), s["d"].data_ptr(), c.n_rays, v.data_ptr(),
                            stream=0 if stream is None else stream.cuda_stream)
    (torch.cuda if stream is None else stream).synchronize()
    return v.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_project_matches_the_model(photon, on_device, name):
    s = on_device(name)
    got, want = project(photon, s, s["f"]), s["Af"]
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{name}: {s['case'].n_rays} rays, {s['case'].taps.ray.size} taps, max |device - model| / max |P| = {err:.2e}, "
          f"{int((got != want).sum())} rays differ")
    assert (got == want).all()                                  # every step is one f64 operation in the model's order
    if name == "random":
        for ray in ("miss_beside", "miss_diagonal", "zero_dir", "nan_origin"):
            assert got[tc.edge_ray(ray)] == 0.0, ray


@pytest.mark.parametrize("name", list(CASES))
def test_backproject_matches_the_model(photon, on_device, name):
    s = on_device(name)
    got, want = backproject(photon, s, s["y"]), s["ATy"]
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{name}: max |device - model| / max |v| = {err:.2e}")
    assert err <= OPERATOR_RTOL


def test_backproject_adds_into_v(photon, on_device):
    s = on_device("random")
    v0 = np.random.default_rng(6).normal(size=s["case"].shape) * np.abs(s["ATy"]).max()
    got, want = backproject(photon, s, s["y"], v0), v0 + s["ATy"]
    assert np.abs(got - want).max() <= OPERATOR_RTOL * np.abs(want).max()
    assert np.abs(got - s["ATy"]).max() > 0.1 * np.abs(want).max()


@pytest.mark.parametrize("name", list(CASES))
def test_adjoint_identity_on_the_device(photon, on_device, name):
    s = on_device(name)
    lhs = float(np.dot(s["y"], project(photon, s, s["f"])))
    rhs = float(np.dot(backproject(photon, s, s["y"]).ravel(), s["f"].ravel()))
    print(f"{name}: <y, A x> = {lhs:.15e}, <A^T y, x> = {rhs:.15e}, relative difference {abs(lhs - rhs) / abs(lhs):.1e}")
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


# ---- "runs": the adjoint's lane merge in exact arithmetic ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    """tc.runs_case on the device with the model's A^T y: every sum is exact (test_tomography.py proves it in rational
    arithmetic), so the device owes the model's bits in whatever order its lanes merge and its atomics land."""
    c = tc.runs_case()
    return dict(case=c, o=dev(c.origins), d=dev(c.dirs), y=c.y, ATy=tm.backproject_model(c.y, *c.grid, c.origins, c.dirs, taps=c.taps))


@pytest.fixture(scope="module")
def side_stream():
    import torch
    return torch.cuda.Stream()


def test_runs_backproject_is_the_model_bit_for_bit(photon, runs):
    got = backproject(photon, runs, runs["y"])
    print(f"runs: {int((got != runs['ATy']).sum())} of {got.size} voxels differ, {int((runs['ATy'] != 0).sum())} are not 0")
    assert np.array_equal(got, runs["ATy"])


def test_runs_backproject_adds_into_whole_numbers_bit_for_bit(photon, runs):
    v0 = tc.whole_numbers(np.random.default_rng(6), runs["case"].shape, top=100)
    got = backproject(photon, runs, runs["y"], v0)
    assert np.array_equal(got, v0 + runs["ATy"])
    assert not np.array_equal(got, runs["ATy"])


def test_runs_project_is_the_model_bit_for_bit(photon, runs):
    c = runs["case"]
    f = np.random.default_rng(17).normal(size=c.shape)
    assert np.array_equal(project(photon, runs, f), tm.project_model(f, c.spacing, c.origin, c.origins, c.dirs, taps=c.taps))


def test_runs_on_a_side_stream(photon, runs, side_stream):
    """The `stream` argument of photon_tomo_project and photon_tomo_backproject: the same bits from a stream of the caller's."""
    c = runs["case"]
    assert np.array_equal(backproject(photon, runs, runs["y"], stream=side_stream), runs["ATy"])
    f = np.random.default_rng(17).normal(size=c.shape)
    assert np.array_equal(project(photon, runs, f, stream=side_stream),
                          tm.project_model(f, c.spacing, c.origin, c.origins, c.dirs, taps=c.taps))


# ---- the solver -------------------------------------------------------------------------------------------------------------
def both(photon, c, p, **kw):
    want, ws = tm.reconstruct_model(p, *c.grid, c.origins, c.dirs, taps=c.taps, **kw)
    got, gs = photon.tomo_reconstruct(p, *c.grid, c.origins, c.dirs, **kw)
    return got, gs, want, ws


def assert_statistics(gs, ws, residual_rtol=RESIDUAL_RTOL):
    """The device's stats against the model's: the whole numbers equal, the residual within residual_rtol of the model's."""
    print(f"stats device {gs}, model {ws}")
    for k in ("iterations", "converged", "unknowns", "rays_used"):
        assert gs[k] == ws[k], (k, gs, ws)
    assert abs(gs["residual"] - ws["residual"]) <= residual_rtol * ws["residual"], (gs, ws)


# CG amplifies the adjoint's summation-order noise on an ill-conditioned problem: with the model's tap order permuted the
# "random" solutions spread by 6e-13 after 10 iterations at lambda 0.5 (1e-5 after 20), and by <= 7e-16 at lambda 50 for any
# count up to 200.  (a) keeps 150x the first spread at 8 iterations, (b) the operators' bound.  The counts (c) to (g) are there
# for the statistics: odd and even, at a check, between checks and none at all, so that the last residual is read from either
# of the solver's two partial arrays; the model's residuals after 0, 1, 7, 8, 9 and 17 iterations at lambda 50 are 1, 0.4169,
# 0.01953, 0.01268, 0.00757 and 1.04e-4: a residual read from the wrong array is off by a factor, the bound (RESIDUAL_RTOL) is
# 550 x the spread of the model's own residual under a permuted tap order, 1.8e-15.
@pytest.mark.parametrize("label,lam,iterations,rtol", [("a", 0.5, 8, 1e-10), ("b", 50.0, 40, 1e-12), ("c", 50.0, 0, 1e-12),
                                                       ("d", 50.0, 1, 1e-12), ("e", 50.0, 7, 1e-12), ("f", 50.0, 9, 1e-12),
                                                       ("g", 50.0, 17, 1e-12)])
def test_fixed_iteration_parity(photon, label, lam, iterations, rtol):
    c = tc.random_case()
    p, w, support = tc.random_problem(c)
    got, gs, want, ws = both(photon, c, p, w=w, support=support, lam=lam, tol=0.0, max_iter=iterations)
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
    """The solver where the adjoint merges lanes.  With the model's tap order permuted the "dense" solution moved by 3.9e-15 of
    max |f| after 8 iterations at lambda 50 (1.5e-14 at lambda 1): the operators' bound keeps 250 x."""
    c = tc.dense_case()
    support = tc.sphere_support(c)
    got, gs, want, ws = both(photon, c, tc.blob_projection(c), w=tc.ray_weights(c.n_rays), support=support, lam=50.0, tol=0.0, max_iter=8)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"dense, lambda 50, 8 iterations: max |device - model| / max |f| = {err:.2e}")
    assert_statistics(gs, ws)
    assert (got[support == 0] == 0).all()
    assert err <= OPERATOR_RTOL


# The dense rays on 2^3, 3^3 and 4^3: every voxel, since the sphere holds 0, 1 and 8 of them, and 2 iterations, since CG on 8
# unknowns ends within 8 (the model's residual after 8 is 2e-10 and moves by its own size under a permuted tap order).  A voxel
# here sums 10^4 to 10^5 taps: with the model's tap order permuted (8 permutations) the solution after 2 iterations moved by at
# most 4.6e-14 of max |f| and the residual by 5.6e-14 of itself.  Both bounds keep 180 x.
COARSE_RTOL = 1e-11


@pytest.mark.parametrize("name", ["coarse2", "coarse3", "coarse4"])
def test_fixed_iteration_parity_with_whole_waves_in_one_voxel(photon, name):
    c = CASES[name]()
    got, gs, want, ws = both(photon, c, tc.blob_projection(c), w=tc.ray_weights(c.n_rays), lam=50.0, tol=0.0, max_iter=2)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{name}, lambda 50, 2 iterations: max |device - model| / max |f| = {err:.2e}")
    assert_statistics(gs, ws, COARSE_RTOL)
    assert gs["iterations"] == 2 and gs["unknowns"] == c.taps.n_voxels
    assert err <= COARSE_RTOL


# ---- the capped grid: more voxels than kMaxBlocks * kThreads = 262 144 -----------------------------------------------------------
# 65^3 = 274 625 voxels: the element-wise kernels of the solver run 1024 blocks whose first 12 481 threads make a second trip,
# and sum_parts sums 1024 partials, four per thread; 64^3 is the cap itself, 1024 blocks and one trip.  4 views of 24^2 rays,
# an odd and an even count.  The voxels of the second trip are the last 12 481, z slabs 62 to 64, and those lie outside the
# sphere: with the sphere support only sum_parts makes the second trip count, so 65^3 runs once more on every voxel (the
# model's solution there reaches 0.35 of max |f|).  With the model's tap order permuted the solutions moved by at most 7.2e-16
# of max |f| and the residuals by 8.6e-16 (every voxel: 6.8e-16 and 1.9e-16): the operators' bound and RESIDUAL_RTOL.
@pytest.mark.parametrize("n,iterations,sphere", [(65, 3, True), (64, 2, True), (65, 3, False)], ids=["65-sphere", "64-sphere", "65-every-voxel"])
def test_fixed_iteration_parity_on_a_capped_grid(photon, n, iterations, sphere):
    c = tc.view_case(n, 24, 4)
    support = tc.sphere_support(c) if sphere else np.ones(c.shape, np.uint8)
    got, gs, want, ws = both(photon, c, tc.blob_projection(c), w=tc.ray_weights(c.n_rays), support=support, lam=50.0, tol=0.0, max_iter=iterations)
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
    1: the check after `stop` iterations ends the run, one iteration before the limit would.  (8, 7): the residual after 7
    iterations would not pass, so the check reads the residual of 8 and not the one before it; (16, 8): the check after 8
    fails and the run goes on."""
    c = tc.random_case()
    p, w, support = tc.random_problem(c)
    kw = dict(w=w, support=support, lam=50.0)
    r = [tm.reconstruct_model(p, *c.grid, c.origins, c.dirs, taps=c.taps, tol=0.0, max_iter=k, **kw)[1]["residual"] for k in (before, stop)]
    tol = float(np.sqrt(r[0] * r[1]))
    assert r[1] < tol < r[0]
    got, gs, want, ws = both(photon, c, p, tol=tol, max_iter=stop + 1, **kw)
    assert_statistics(gs, ws)
    assert gs["iterations"] == stop and gs["converged"] == 1
    assert np.abs(got - want).max() <= OPERATOR_RTOL * np.abs(want).max()


def test_an_empty_support_needs_no_iteration(photon):
    c = tc.random_case()
    p, w, _ = tc.random_problem(c)
    got, gs, want, ws = both(photon, c, p, w=w, support=np.zeros(c.shape, np.uint8), lam=50.0, tol=0.0, max_iter=9)
    assert_statistics(gs, ws)
    assert gs["iterations"] == 0 and gs["unknowns"] == 0 and gs["converged"] == 1 and gs["residual"] == 0.0
    assert (got == 0).all() and (want == 0).all()


def test_pointer_form_on_a_side_stream(photon, side_stream):
    """tomo_reconstruct_ptr on device tensors and a stream of the caller's against the array form and the model."""
    import torch
    c = tc.random_case()
    p, w, support = tc.random_problem(c)
    kw = dict(lam=50.0, tol=0.0, max_iter=9)
    _, array_stats, want, ws = both(photon, c, p, w=w, support=support, **kw)
    dp, dw, ds, do, dd = dev(p), dev(w), dev(support), dev(c.origins), dev(c.dirs)
    f = torch.full(c.shape, 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gs = photon.tomo_reconstruct_ptr(dp.data_ptr(), *c.grid, do.data_ptr(), dd.data_ptr(), c.n_rays, f.data_ptr(), d_w_ptr=dw.data_ptr(),
                                     d_support_ptr=ds.data_ptr(), stream=side_stream.cuda_stream, **kw)
    got = f.cpu().numpy()                                       # the call has synchronised its stream
    for k in ("iterations", "converged", "unknowns", "rays_used"):
        assert gs[k] == array_stats[k], (k, gs, array_stats)
    assert_statistics(gs, ws)
    assert (got[support == 0] == 0).all()
    assert np.abs(got - want).max() <= OPERATOR_RTOL * np.abs(want).max()


def test_converged_parity(photon):
    c = tc.random_case()
    p, w, support = tc.random_problem(c)
    got, gs, want, ws = both(photon, c, p, w=w, support=support, lam=5.0, tol=1e-10, max_iter=2000)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"(c) lambda 5, tol 1e-10: device {gs['iterations']} iterations, model {ws['iterations']}; max |device - model| / max |f| = "
          f"{err:.2e}")
    assert gs["converged"] == 1 and ws["converged"] == 1
    assert abs(gs["iterations"] - ws["iterations"]) <= tm.CHECK_EVERY
    assert err <= 1e-7


def test_views_reconstruct_the_blob(photon):
    c = tc.views_case()
    truth, p = tc.blob_field(c), tc.blob_projection(c)
    f, st = photon.tomo_reconstruct(p, *c.grid, c.origins, c.dirs, lam=1.0, tol=0.0, max_iter=50)
    support = tc.sphere_support(c)
    fs, sts = photon.tomo_reconstruct(p, *c.grid, c.origins, c.dirs, support=support, lam=1.0, tol=0.0, max_iter=50)
    e, es = tc.rel_l2(f, truth), tc.rel_l2(fs, truth)
    print(f"(d) views on the device: relative L2 error {e:.4f} (bound 0.05), inside the sphere {es:.4f} (bound 0.03)")
    assert st["iterations"] == 50 and st["unknowns"] == 24 ** 3 and st["rays_used"] == c.n_rays
    assert sts["unknowns"] == int(support.sum()) and (fs[support == 0] == 0).all()
    assert e <= 0.05
    assert es <= 0.03


def test_zero_data_needs_no_iteration(photon):
    c = tc.random_case()
    f, st = photon.tomo_reconstruct(np.zeros(c.n_rays), *c.grid, c.origins, c.dirs)
    assert st["iterations"] == 0 and st["converged"] == 1 and st["residual"] == 0.0 and (f == 0).all()


def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    n = 8
    rays = torch.ones((n, 3), dtype=torch.float64, device="cuda")
    vals = torch.zeros((n,), dtype=torch.float64, device="cuda")
    out = torch.full((4, 4, 4), 7.0, dtype=torch.float64, device="cuda")
    outp = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    r, v, o, op = (ctypes.c_void_p(t.data_ptr()) for t in (rays, vals, out, outp))
    nan, inf = float("nan"), float("inf")
    arr = lambda *x: (ctypes.c_double * 3)(*x)      # noqa: E731
    sp, og = arr(1.0, 1.0, 1.0), arr(0.0, 0.0, 0.0)
    good = dict(nx=4, ny=4, nz=4, sp=sp, og=og, o=r, d=r, n=n)
    grid_cases = [("nx 1", dict(nx=1)), ("ny 1", dict(ny=1)), ("nz 1", dict(nz=1)), ("too many voxels", dict(nx=2048, ny=2048, nz=2048)),
                  ("no rays", dict(n=0)), ("spacing 0", dict(sp=arr(1.0, 0.0, 1.0))), ("spacing < 0", dict(sp=arr(-1.0, 1.0, 1.0))),
                  ("spacing nan", dict(sp=arr(1.0, 1.0, nan))), ("spacing inf", dict(sp=arr(inf, 1.0, 1.0))),
                  ("origin nan", dict(og=arr(0.0, nan, 0.0))), ("origin inf", dict(og=arr(0.0, 0.0, inf))),
                  ("null spacing", dict(sp=None)), ("null origin", dict(og=None)),
                  ("null origins", dict(o=None)), ("null dirs", dict(d=None))]

    def grid_args(g):
        return (g["nx"], g["ny"], g["nz"], g["sp"], g["og"], g["o"], g["d"], g["n"])

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
        check("photon_tomo_project", what, L.photon_tomo_project(o, *grid_args(g), op, None))
        check("photon_tomo_backproject", what, L.photon_tomo_backproject(v, *grid_args(g), o, None))
    check("photon_tomo_project", "null d_f", L.photon_tomo_project(None, *grid_args(good), op, None))
    check("photon_tomo_project", "null d_p", L.photon_tomo_project(o, *grid_args(good), None, None))
    check("photon_tomo_backproject", "null d_y", L.photon_tomo_backproject(None, *grid_args(good), o, None))
    check("photon_tomo_backproject", "null d_v", L.photon_tomo_backproject(v, *grid_args(good), None, None))
    solver_cases = grid_cases + [("lambda < 0", dict(lam=-1.0)), ("lambda nan", dict(lam=nan)), ("tol < 0", dict(tol=-1.0)),
                                 ("tol nan", dict(tol=nan)), ("max_iter < 0", dict(it=-1)), ("null p", dict(p=None)), ("null f", dict(f=None))]
    for what, change in solver_cases:
        g = {**good, **dict(lam=1.0, tol=1e-6, it=10, p=v, f=o), **change}
        st = photon_tomo_stats_t(-5, -5, -5, -5, -5.0)
        rc = L.photon_tomo_reconstruct(g["p"], None, None, *grid_args(g), g["lam"], g["tol"], g["it"], g["f"], ctypes.byref(st), None)
        check("photon_tomo_reconstruct", what, rc, st)
    c = tc.random_case()                                                              # accepted calls are silent
    f, st = photon.tomo_reconstruct(np.ones(c.n_rays), *c.grid, c.origins, c.dirs, max_iter=3)
    assert capfd.readouterr().err == "" and st["iterations"] == 3
