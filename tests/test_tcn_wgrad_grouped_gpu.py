"""GPU: the grouped, split-free TN launch of the TCN weight gradients (csrc/tcn.hip gemm_tn_grouped_kernel, C ABI
nppc_gemm_tn_grouped) against fp64 products of the bf16-rounded operands.

No tolerance is picked here: the same inputs also go through the path this launch replaces (nppc_gemm_tn_splitk_batched +
nppc_reduce_slabs / nppc_reduce_slabs_t, ksplit = 8 where R allows it, else the largest R allows).  Both accumulate the same
exact bf16 products in fp32 and differ only in the order of the additions, so the grouped launch's largest error against
fp64 may be at most twice the replaced path's.  Both errors of every shape go to profiles/tcn_wgrad_grouped_errors.json (the
entries of the shapes that ran are replaced, the others kept; the sums are deterministic, so a rerun leaves the file as it
is).  (One running sum over all rows missed that bound: 2.5e-5 against 9.4e-6 at
M = 128, ldC = 64, R = 192, six problems, transposed.  The kernel therefore sums the rows in the same blocks as the split
launches and adds the block sums in their order, which makes the two paths agree bit for bit at these shapes; that is
asserted as well.)

Shapes: the smallest at which each mechanism can go wrong -- one and two row tiles (M = 128, 256); clipping inside one
column tile (ldC = 64, C = 37) and a whole tile plus a clipped one (ldC = 192, C = 130); one stage (R = 64: prologue only)
and three (R = 192: prologue, steady state, drain of the double buffer); tables of 1 and 6 problems; both store kinds.
The operands are exact-size tensors, the destinations dense slices of ONE flat fp32 buffer that holds a sentinel everywhere
else: nothing but the destinations may change, and every destination element must be written."""
import itertools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
SENT = -12345.0
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ERRORS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    if _ERRORS:
        path = os.path.join(REPO, "profiles", "tcn_wgrad_grouped_errors.json")
        try:
            with open(path) as f:
                kept = json.load(f)
        except (OSError, ValueError):
            kept = {}
        kept.update(_ERRORS)
        try:
            with open(path, "w") as f:
                json.dump(kept, f, indent=1, sort_keys=True)
        except OSError:
            pass                                   # a read-only checkout: the record is a by-product, not the check


def _ksplit(R):
    return max(k for k in range(1, 9) if R % (64 * k) == 0)


CASES = [pytest.param(M, ldC, C, R, nprob, kind, id=f"M{M}-ld{ldC}-C{C}-R{R}-n{nprob}-{'t' if kind else 'asis'}")
         for M, (ldC, C), R, nprob, kind in itertools.product((128, 256), ((64, 37), (192, 130)), (64, 192), (1, 6), (0, 1))]


@pytest.mark.parametrize("M,ldC,C,R,nprob,kind", CASES)
def test_grouped_tn_matches_fp64_like_the_split_path(M, ldC, C, R, nprob, kind):
    from nppc_audio import _hip as H
    g = torch.Generator().manual_seed(1000 * M + 10 * ldC + R + nprob + kind)
    # per problem: A [R][M], B [R][ldC] (padding columns C.. hold values too: they must never reach a destination)
    a = [(torch.randn(R, M, generator=g) * 2.0 ** (p % 3 - 1)).bfloat16() for p in range(nprob)]
    b = [torch.randn(R, ldC, generator=g).bfloat16() for p in range(nprob)]
    ref = [a[p].double().t() @ b[p].double()[:, :C] for p in range(nprob)]                  # [M][C]
    if kind == H.TN_STORE_TRANSPOSED:
        ref = [r.t().contiguous() for r in ref]                                            # [C][M]
    dst_ld = M if kind == H.TN_STORE_TRANSPOSED else C
    n_dst = M * C
    gap = 77                                                                               # odd: unaligned destinations
    offs = [gap + p * (n_dst + gap) for p in range(nprob)]
    total = offs[-1] + n_dst + gap
    A = [t.cuda() for t in a]
    B = [t.cuda() for t in b]
    s = H.stream()

    def grouped():
        flat = torch.full((total,), SENT, device="cuda")
        tab = H.tn_problem_table([(A[p], M, B[p], ldC, flat[offs[p]: offs[p] + n_dst], dst_ld, C, kind) for p in range(nprob)],
                                 M, ldC, R)
        H.call("nppc_gemm_tn_grouped", tab, nprob, M, ldC, R, s)
        torch.cuda.synchronize()
        return flat.cpu()

    def split():
        S = _ksplit(R)
        flat = torch.full((total,), SENT, device="cuda")
        slab = torch.empty(S * M * ldC, device="cuda")
        for p in range(nprob):
            dst = flat[offs[p]: offs[p] + n_dst]
            H.call("nppc_gemm_tn_splitk_batched", A[p], M, 0, B[p], ldC, 0, slab, ldC, 0, M, ldC, R, S, 1, s)
            if kind == H.TN_STORE_TRANSPOSED:
                H.call("nppc_reduce_slabs_t", slab, S, M * ldC, ldC, dst, M, C, M, 0, 0, 1, s)
            else:
                H.call("nppc_reduce_slabs", slab, S, M * ldC, ldC, dst, C, M, 0, C, 0, 0, 0, 0, 1, s)
        torch.cuda.synchronize()
        return flat.cpu()

    def max_err(flat):
        return max(float((flat[offs[p]: offs[p] + n_dst].double() - ref[p].reshape(-1)).abs().max()) for p in range(nprob))

    got, again, old = grouped(), grouped(), split()
    inside = torch.zeros(total, dtype=torch.bool)
    for o in offs:
        inside[o: o + n_dst] = True
    assert bool((got[~inside] == SENT).all()), "a store outside the destinations"
    assert bool((got[inside] != SENT).all()), "a destination element was not written"
    assert torch.equal(got, again), "two launches on the same inputs differ"
    e_new, e_old = max_err(got), max_err(old)
    _ERRORS[f"M{M}_ldC{ldC}_C{C}_R{R}_n{nprob}_kind{kind}"] = {"grouped_max_abs_err": e_new, "split_max_abs_err": e_old,
                                                              "ksplit": _ksplit(R)}
    print(f"grouped {e_new:.3e}  split(ksplit={_ksplit(R)}) {e_old:.3e}")
    assert e_new <= 2.0 * e_old, (e_new, e_old)
    assert torch.equal(got, old), "the blocked sums are not the split path's bits"


def test_grouped_tn_rejects_bad_arguments():
    from nppc_audio import _hip as H
    tab = torch.zeros(1, 8, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_gemm_tn_grouped", tab, 0, 128, 64, 64, H.stream())
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_gemm_tn_grouped", None, 1, 128, 64, 64, H.stream())
    for M, N, R in ((64, 64, 64), (128, 32, 64), (128, 64, 96)):
        with pytest.raises(RuntimeError, match="unsupported"):
            H.call("nppc_gemm_tn_grouped", tab, 1, M, N, R, H.stream())
