"""fp64 / complex128 references of the Gram-Schmidt and NPPC-loss algebra in csrc/gsloss.hip, written from its comments.

A vector set is [B][K][2][N] (real and imaginary planes); with gt / pred the set gains e = gt - pred as index K.  The kernel
forms e in fp32: `vec_set` subtracts in the dtype it is given, so fp32 gt / pred give the kernel's e and every Gram product
of fp32 inputs is exact in fp64.  Coefficient matrices are complex128 [B][KV][KV]; `to_planes` / `from_planes` convert from /
to the kernel's [B][KV][KV][2] fp64 layout.
tests/test_gsloss_ref_cpu.py checks that these functions, composed, reproduce oracle/nppc_ref.py and oracle/inpaint_ref.py
run in fp64, values and autograd gradients."""
import torch


def cplx(x):
    """[..., 2, N] real planes (any float dtype) -> complex128 [..., N]"""
    x = x.double()
    return torch.complex(x[..., 0, :], x[..., 1, :])


def vec_set(v, gt=None, pred=None):
    """[B][K][2][N] (+ gt, pred [B][2][N]) -> complex128 [B][KV][N], e = gt - pred (in the inputs' dtype) at index K"""
    z = cplx(v)
    if gt is None:
        return z
    e = (gt - pred).reshape(gt.shape[0], 2, -1)
    return torch.cat([z, cplx(e)[:, None]], dim=1)


def to_planes(M):
    """complex128 [B][KV][KV] -> fp64 [B][KV][KV][2]"""
    return torch.view_as_real(M.contiguous()).contiguous()


def from_planes(M):
    """fp64 [B][KV][KV][2] -> complex128 [B][KV][KV]"""
    return torch.view_as_complex(M.double().contiguous())


def gram(a, b=None):
    """G[b][i][n] = <a_i, b_n> = sum_t conj(a_i[t]) b_n[t] on complex sets [B][KV][N]; b = None: the same set"""
    b = a if b is None else b
    return torch.einsum("bit,bnt->bin", a.conj(), b)


def gram_mag(a, b=None):
    """S[b][i][n] = sum_t |a_i[t]| |b_n[t]|: the scale of the summation error bound of gram()"""
    b = a if b is None else b
    return torch.einsum("bit,bnt->bin", a.abs(), b.abs())


def combine(M1, A, M2=None, Bv=None):
    """out_i = sum_m M1[i][m] A_m (+ sum_m M2[i][m] B_m), complex sets [B][KV][N] -> [B][KV][N] (rows i >= K unused)"""
    out = torch.einsum("bim,bmt->bit", M1, A)
    if M2 is not None:
        out = out + torch.einsum("bim,bmt->bit", M2, Bv)
    return out


def gdot(a, bv, G):
    """<sum_m a_m x_m, sum_n b_n x_n> = sum_{m,n} conj(a_m) b_n G[m][n]"""
    return (a.conj()[:, None] * bv[None, :] * G).sum()


def gs_solve(G, K):
    """Gram-Schmidt in coefficient space (gsloss.hip gs_solve_kernel): w_i = sum_m C[i][m] x_m, w_hat_i = sum_m Ch[i][m] x_m.
      C_i = e_i - sum_{j<i} <w_i, w_hat_j> Ch_j   (the running w_i, the coefficient conj(w) . w_hat of the reference)
      Ch_i = C_i / sqrt(<w_i, w_i>)
    G: complex128 [B][KV][KV] (KV >= K, only the leading K x K is read).  Returns C, Ch as complex128 [B][K][K]."""
    B = G.shape[0]
    C = torch.zeros(B, K, K, dtype=torch.complex128)
    Ch = torch.zeros_like(C)
    for b in range(B):
        g = G[b, :K, :K]
        for i in range(K):
            c = torch.zeros(K, dtype=torch.complex128)
            c[i] = 1.0
            for j in range(i):
                c = c - gdot(c, Ch[b, j], g) * Ch[b, j]
            C[b, i] = c
            Ch[b, i] = c / torch.sqrt(gdot(c, c, g).real)
    return C, Ch


def gs_bwd_solve(G, P, Ch, K):
    """Backward of Gram-Schmidt with w_hat detached (gsloss.hip gs_bwd_solve_kernel):
      dx_i = A_0^T .. A_{i-1}^T g_i,  A_j^T(u) = u - w_hat_j <u, w_hat_j>;  with u = g_i + sum_m d_m x_m, j = i-1 .. 0:
      d <- d - (sum_n Ch[j][n] P[i][n] + sum_{m,n} conj(d_m) Ch[j][n] G[m][n]) Ch_j,   P[i][n] = <g_i, x_n>.
    Returns D as complex128 [B][K][K]: dx_i = g_i + sum_m D[i][m] x_m."""
    B = G.shape[0]
    D = torch.zeros(B, K, K, dtype=torch.complex128)
    for b in range(B):
        g = G[b, :K, :K]
        for i in range(K):
            d = torch.zeros(K, dtype=torch.complex128)
            for j in range(i - 1, -1, -1):
                s = (Ch[b, j] * P[b, i, :K]).sum() + gdot(d, Ch[b, j], g)
                d = d - s * Ch[b, j]
            D[b, i] = d
    return D


def loss_solve(G, K, eps=1e-8, eps_in_norms=0, lam=None):
    """The loss scalars from the Gram of [w_0 .. w_{K-1}, e] (KV = K + 1), gsloss.hip loss_solve_kernel, all fp64:
      en = |e|, de = en + eps, wn_i = |w_i|, dw_i = wn_i + eps, q_i = <w_i, e>, proj_i = q_i / (dw_i de),
      wno_i = (eps_in_norms ? dw_i : wn_i) / de, reconst = 1 - sum_i |proj_i|^2, sm_i = (wno_i^2 - |proj_i|^2)^2,
      coefA[i] = (d|proj|^2/dw : w part, d sm/dw : w part), coefE[i] = d|proj|^2/dw : e part = 2 conj(q) / (dw^2 de^2).
    Returns a dict of fp64 tensors ([B] or [B][K]; coefA [B][K][2], coefE complex [B][K]).  With lam: also the objective
    mean(reconst) + lam mean(sm) of the fp64 values."""
    G = G[:, :K + 1, :K + 1]
    en = torch.sqrt(G[:, K, K].real)
    de = en + eps
    idx = torch.arange(K)
    wn = torch.sqrt(G[:, idx, idx].real)
    dw = wn + eps
    q = G[:, idx, K]
    proj = q / (dw * de[:, None])
    pm2 = proj.real ** 2 + proj.imag ** 2
    wno = (dw if eps_in_norms else wn) / de[:, None]
    dsm = wno * wno - pm2
    wsafe = torch.where(wn > 0, wn, torch.ones_like(wn))
    d2 = de[:, None] ** 2
    coefA = torch.stack([-2.0 * q.abs() ** 2 / (dw ** 3 * d2) / wsafe, 4.0 * dsm * wno / (de[:, None] * wsafe)], dim=-1)
    coefE = 2.0 * q.conj() / (dw ** 2 * d2)
    out = dict(err_norm=de if eps_in_norms else en, proj=proj, proj_mag=torch.sqrt(pm2), w_norms=wno,
               reconst=1.0 - pm2.sum(dim=1), sm=dsm * dsm, coefA=coefA, coefE=coefE)
    if lam is not None:
        out["objective"] = out["reconst"].mean() + lam * out["sm"].mean()
    return out


def loss_bwd_coef(coefA, coefE, grec, gobj_over_B, gsm, K):
    """M1 (complex128 [B][K+1][K+1]) with dL/dw_i = sum_m M1[i][m] [w, e]_m  (gsloss.hip loss_bwd_coef_kernel):
      M1[i][i] = -gr_b coefA[i][0] + gsm coefA[i][1],  M1[i][K] = -gr_b coefE[i],  gr_b = gobj_over_B + grec[b]."""
    B = coefA.shape[0]
    gr = torch.full((B,), float(gobj_over_B), dtype=torch.float64)
    if grec is not None:
        gr = gr + grec.double()
    M = torch.zeros(B, K + 1, K + 1, dtype=torch.complex128)
    idx = torch.arange(K)
    M[:, idx, idx] = (-gr[:, None] * coefA[..., 0] + gsm * coefA[..., 1]).to(torch.complex128)
    M[:, idx, K] = -gr[:, None] * coefE
    return M


def gram_schmidt(x):
    """The Gram-Schmidt forward through the coefficient solve: [B][K][2][F][T] -> w (complex128 [B][K][N]), C, Ch, G"""
    B, K = x.shape[:2]
    z = vec_set(x.reshape(B, K, 2, -1))
    G = gram(z)
    C, Ch = gs_solve(G, K)
    return combine(C, z), C, Ch, G


def gram_schmidt_bwd(x, gy):
    """dx (complex128 [B][K][N]) for upstream gy [B][K][2][F][T]"""
    B, K = x.shape[:2]
    z = vec_set(x.reshape(B, K, 2, -1))
    g = vec_set(gy.reshape(B, K, 2, -1))
    G = gram(z)
    _, Ch = gs_solve(G, K)
    D = gs_bwd_solve(G, gram(g, z), Ch, K)
    return g + combine(D, z)


def nppc_loss(w, gt, pred, lam, eps=1e-8, eps_in_norms=0, grec=None, gobj=1.0):
    """Loss forward and the gradient dw (complex128 [B][K][N]) for upstream grec [B] (or None) and gobj, as NPPCLoss
    applies them (gobj / B on reconst, gobj lam / (B K) on sm)"""
    B, K = w.shape[:2]
    z = vec_set(w.reshape(B, K, 2, -1), gt.reshape(B, 2, -1), pred.reshape(B, 2, -1))
    out = loss_solve(gram(z), K, eps, eps_in_norms, lam)
    M1 = loss_bwd_coef(out["coefA"], out["coefE"], grec, gobj / B, gobj * lam / (B * K), K)
    out["dw"] = combine(M1, z)[:, :K]
    return out
