"""CPU: the fp64 references of tests/gsloss_ref.py, composed (Gram -> coefficient solve -> combination), reproduce the
oracles run in fp64 (oracle/nppc_ref.py gram_schmidt_crm / nppc_loss, oracle/inpaint_ref.py gram_schmidt_real /
inpaint_loss), values and autograd gradients.  tests/test_gsloss_paths_gpu.py measures the HIP kernels against these
references, so they are checked here first.

The two sides differ only in the order of fp64 operations: the oracle projects the vectors, the reference solves for
coefficients on the Gram matrix.  Both are backward-stable on well-conditioned inputs, so 1e-12 relative is far above the
~1e-15 they agree to and far below any fp32 effect."""
import pytest
import torch

import gsloss_ref as GR
from oracle import inpaint_ref as IR
from oracle import nppc_ref as R

TOL = 1e-12


def rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def inputs(B, K, F, T, seed, collinear=None):
    """fp32-representable fp64 vectors; collinear = (j, delta): x_j = x_0 + delta * noise"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, 2, F, T, generator=g)
    if collinear is not None:
        j, d = collinear
        x[:, j] = x[:, 0] + d * torch.randn(B, 2, F, T, generator=g)
    return x.double(), torch.randn(B, K, 2, F, T, generator=g).double()


@pytest.mark.parametrize("B,K,F,T,coll", [(2, 1, 5, 7, None), (3, 2, 9, 11, None), (2, 5, 16, 9, None),
                                          (2, 8, 8, 12, None), (1, 9, 10, 10, None), (2, 4, 16, 16, (3, 1e-3))])
def test_gram_schmidt_ref_matches_oracle(B, K, F, T, coll):
    x, gy = inputs(B, K, F, T, 10 * K + B, coll)
    xr = x.clone().requires_grad_(True)
    w = R.gram_schmidt_crm(xr)
    (w * gy).sum().backward()
    got, _, _, _ = GR.gram_schmidt(x)
    want = GR.cplx(w.detach().reshape(B, K, 2, -1))
    # conditioning of the collinear pair (1/delta) enters both sides' fp64 rounding
    tol = TOL if coll is None else TOL / coll[1]
    assert rel(got, want) < tol
    assert rel(GR.gram_schmidt_bwd(x, gy), GR.cplx(xr.grad.reshape(B, K, 2, -1))) < tol


def test_gram_schmidt_ref_matches_real_oracle():
    g = torch.Generator().manual_seed(7)
    B, K, F, T = 3, 4, 12, 10
    x = torch.randn(B, K, F, T, generator=g).double()
    gy = torch.randn(B, K, F, T, generator=g).double()
    xr = x.clone().requires_grad_(True)
    w = IR.gram_schmidt_real(xr)
    (w * gy).sum().backward()
    planes = lambda v: torch.stack([v, torch.zeros_like(v)], dim=2)
    got, _, _, _ = GR.gram_schmidt(planes(x))
    assert rel(got.real, w.detach().reshape(B, K, -1)) < TOL
    assert float(got.imag.abs().max()) == 0.0
    dx = GR.gram_schmidt_bwd(planes(x), planes(gy))
    assert rel(dx.real, xr.grad.reshape(B, K, -1)) < TOL
    assert float(dx.imag.abs().max()) == 0.0


def test_gs_solve_is_triangular_and_normalised():
    x, _ = inputs(2, 6, 8, 8, 3)
    _, C, Ch, G = GR.gram_schmidt(x)
    # C lower triangular with a unit diagonal; every w_hat has unit norm.  (The complex rows are not orthogonal: the
    # reference's coefficient is <w, w_hat>, not <w_hat, w>.)  Real vectors: the w_hat are orthonormal.
    assert float(torch.triu(C, 1).abs().max()) == 0.0
    assert float((torch.diagonal(C, dim1=1, dim2=2) - 1).abs().max()) == 0.0
    H = Ch.conj() @ G @ Ch.transpose(1, 2)
    assert float((torch.diagonal(H, dim1=1, dim2=2) - 1).abs().max()) < TOL
    xr = x.clone()
    xr[:, :, 1] = 0
    _, _, Ch, G = GR.gram_schmidt(xr)
    eye = torch.eye(6, dtype=torch.complex128).expand(2, 6, 6)
    assert rel(Ch.conj() @ G @ Ch.transpose(1, 2), eye) < TOL


@pytest.mark.parametrize("B,K,F,T,step", [(4, 3, 16, 9, 0), (4, 5, 12, 11, 250), (2, 8, 9, 9, 500), (65, 2, 4, 5, 375)])
def test_nppc_loss_ref_matches_oracle(B, K, F, T, step):
    g = torch.Generator().manual_seed(step + K)
    w = (torch.randn(B, K, 2, F, T, generator=g) * 0.3).double()
    gt = torch.randn(B, 2, F, T, generator=g).double()
    pred = torch.randn(B, 2, F, T, generator=g).double()
    wr = w.clone().requires_grad_(True)
    rec_r, obj_r, log = R.nppc_loss(wr, gt, pred, step)
    grec = torch.linspace(0.5, 1.5, B, dtype=torch.float64)
    (obj_r + (rec_r * grec).sum()).backward()
    lam = R.second_moment_weight(step)
    got = GR.nppc_loss(w, gt, pred, lam, grec=grec)
    assert abs(float(got["objective"] - obj_r)) < TOL
    assert rel(got["reconst"], rec_r.detach()) < TOL
    assert rel(got["err_norm"], log["err_norm"]) < TOL
    assert rel(got["proj"], log["err_proj"]) < TOL
    assert rel(got["proj_mag"], log["err_proj_mag"]) < TOL
    assert rel(got["w_norms"], log["w_norms"]) < TOL
    assert rel(got["sm"], log["second_moment_mse"]) < TOL
    assert rel(got["dw"], GR.cplx(wr.grad.reshape(B, K, 2, -1))) < TOL


@pytest.mark.parametrize("backprop", ["both", "reconst", "objective"])
def test_inpaint_loss_ref_matches_oracle(backprop):
    g = torch.Generator().manual_seed(11)
    B, K, F, T, step = 4, 5, 16, 12, 300
    w = (torch.randn(B, K, F, T, generator=g) * 0.2).double()
    w[:, :, :, :4] = 0.0                                   # zero outside the gap, as the trainer leaves them
    clean = torch.randn(B, F, T, generator=g).double()
    pred = torch.randn(B, F, T, generator=g).double()
    wr = w.clone().requires_grad_(True)
    rec_r, obj_r, log = IR.inpaint_loss(wr, clean, pred, step)
    grec = torch.linspace(-1.0, 2.0, B, dtype=torch.float64)
    loss = {"both": obj_r + (rec_r * grec).sum(), "reconst": (rec_r * grec).sum(), "objective": obj_r}[backprop]
    loss.backward()
    lam = IR.second_moment_weight(step)
    planes = lambda v: torch.stack([v, torch.zeros_like(v)], dim=-3)
    got = GR.nppc_loss(planes(w), planes(clean), planes(pred), lam, eps=1e-6, eps_in_norms=1,
                       grec=None if backprop == "objective" else grec, gobj=0.0 if backprop == "reconst" else 1.0)
    assert abs(float(got["objective"] - obj_r)) < TOL
    assert rel(got["reconst"], rec_r.detach()) < TOL
    assert rel(got["err_norm"], log["err_norm"]) < TOL
    assert rel(got["proj"].real, log["err_proj"]) < TOL
    assert float(got["proj"].imag.abs().max()) == 0.0
    assert rel(got["w_norms"], log["w_norms"]) < TOL
    assert rel(got["sm"], log["second_moment_mse"]) < TOL
    assert rel(got["dw"].real, wr.grad.reshape(B, K, -1)) < TOL
    assert float(got["dw"].imag.abs().max()) == 0.0
