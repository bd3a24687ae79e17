"""Section 9 on the GPU (include/parallel_ray_tracing.h): photon_tomo_project, photon_tomo_backproject and
photon_tomo_reconstruct against the f64 host model of photon_amd/tomography.py on the shared cases of tomography_cases.py,
the adjoint identity on the device, the solver's parity at fixed iteration counts and at convergence, the blob
reconstructed from its views, and the refusals."""
import ctypes

import numpy as np
import pytest

import tomography_cases as tc
from photon_amd import tomography as tm
from photon_amd.library import photon_tomo_stats_t

pytestmark = pytest.mark.gpu

# project: the device runs the model's operations in the model's order; backproject: only the order of a voxel's sum
# differs (a permuted order moved the model by 4e-16 of max |v|).  Both bounds are relative to the largest output.
OPERATOR_RTOL = 1e-12

# "dense": four rays per voxel and axis, so that runs of up to six adjacent lanes add to one voxel and the adjoint's merge of
# such lanes runs its steps of distance 1, 2 and 4 (test_tomography.py holds the run length); the other cases stop at two.
CASES = {"random": tc.random_case, "views": tc.views_case, "large": tc.large_case, "dense": tc.dense_case}


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


def project(photon, s, f):
    import torch
    c = s["case"]
    p = torch.full((c.n_rays,), 7.0, dtype=torch.float64, device="cuda")
    photon.tomo_project(dev(f).data_ptr(), *c.grid, s["o"].data_ptr(), s["d"].data_ptr(), c.n_rays, p.data_ptr())
    torch.cuda.synchronize()
    return p.cpu().numpy()


def backproject(photon, s, y, v0=None):
    import torch
    c = s["case"]
    v = torch.zeros(c.shape, dtype=torch.float64, device="cuda") if v0 is None else dev(v0)
    photon.tomo_backproject(dev(y).data_ptr(), *c.grid, s["o"].data_ptr(), s["d"].data_ptr(), c.n_rays, v.data_ptr())
    torch.cuda.synchronize()
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


# ---- the solver -------------------------------------------------------------------------------------------------------------
def both(photon, c, p, **kw):
    want, ws = tm.reconstruct_model(p, *c.grid, c.origins, c.dirs, taps=c.taps, **kw)
    got, gs = photon.tomo_reconstruct(p, *c.grid, c.origins, c.dirs, **kw)
    return got, gs, want, ws


# CG amplifies the adjoint's summation-order noise on an ill-conditioned problem: with the model's tap order permuted the
# "random" solutions spread by 6e-13 after 10 iterations at lambda 0.5 (1e-5 after 20), and by <= 7e-16 at lambda 50 for any
# count up to 200.  (a) keeps 150x the first spread at 8 iterations, (b) the operators' bound.
@pytest.mark.parametrize("label,lam,iterations,rtol", [("a", 0.5, 8, 1e-10), ("b", 50.0, 40, 1e-12)])
def test_fixed_iteration_parity(photon, label, lam, iterations, rtol):
    c = tc.random_case()
    p, w, support = tc.random_problem(c)
    got, gs, want, ws = both(photon, c, p, w=w, support=support, lam=lam, tol=0.0, max_iter=iterations)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"({label}) lambda {lam}, {iterations} iterations: max |device - model| / max |f| = {err:.2e}; residual device "
          f"{gs['residual']:.3e}, model {ws['residual']:.3e}")
    for k in ("iterations", "unknowns", "rays_used"):
        assert gs[k] == ws[k], (k, gs, ws)
    assert gs["iterations"] == iterations and gs["unknowns"] == int(support.sum())
    assert (got[support == 0] == 0).all()
    assert err <= rtol


def test_fixed_iteration_parity_with_dense_rays(photon):
    """The solver where the adjoint merges lanes.  With the model's tap order permuted the "dense" solution moved by 3.9e-15 of
    max |f| after 8 iterations at lambda 50 (1.5e-14 at lambda 1): the operators' bound keeps 250 x."""
    c = tc.dense_case()
    rng = np.random.default_rng(9)
    p = tc.blob_projection(c)
    w = rng.uniform(0.2, 2.0, p.shape)
    w[rng.random(p.shape) < 0.1] = 0.0
    support = tc.sphere_support(c)
    got, gs, want, ws = both(photon, c, p, w=w, support=support, lam=50.0, tol=0.0, max_iter=8)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"dense, lambda 50, 8 iterations: max |device - model| / max |f| = {err:.2e}")
    for k in ("iterations", "unknowns", "rays_used"):
        assert gs[k] == ws[k], (k, gs, ws)
    assert (got[support == 0] == 0).all()
    assert err <= OPERATOR_RTOL


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
