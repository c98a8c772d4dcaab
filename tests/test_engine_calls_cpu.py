"""CPU: the keyword launch wrappers of nppc_audio/gemm.py and nppc_audio/unet_engine.py emit the positional lists of the C ABI
(`_hip.SIGS`), and `lstm_wgrad_mode` picks the LSTM weight-gradient strategy by the conditions FSNEngine._lstm_wgrad has always used."""
import pytest

from nppc_audio import _hip as H
from nppc_audio import gemm
from nppc_audio import unet_engine as UE
from nppc_audio.engine import (EPI_MASK_POS, EPI_PLAIN_F32, EPI_PRELU_STATS, EPI_RESIDUAL, TCN_HIDDEN)
from nppc_audio.ops_lstm import WGRAD_SPLITS


class _T:
    """stands for a device tensor: the wrappers must hand it on untouched"""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return f"<{self.name}>"


@pytest.fixture
def calls(monkeypatch):
    out = []
    monkeypatch.setattr(H, "call", lambda name, *args: out.append((name, list(args))))
    return out


def _check_kinds(name, args):
    sig = H.SIGS[name]
    assert len(args) == len(sig), (name, len(args), len(sig))
    for k, (a, t) in enumerate(zip(args, sig)):
        if t is H.P:
            assert a is None or isinstance(a, _T), (name, k, a)
        elif t in (H.I, H.L):
            assert type(a) is int, (name, k, a)
        else:
            assert t in (H.F, H.D) and type(a) is float, (name, k, a)


A, B, C, RES, BIAS, SLOPE, STATS, CP, S, U, V, DST = (_T(n) for n in "A B C res bias slope stats colpart stream u v dst".split())
NT = dict(A=(A, 320, 1000), B=(B, 320, 2000), C=(C, 512, 3000), R=256, N=512, K=320, Tp=128, Tv=101, Nv=500, stream=S)


@pytest.mark.parametrize("kw", [
    dict(),
    dict(bias=(BIAS, 7), res=(RES, 512, 3000), slope=(SLOPE, 7), stats=(STATS, 4), relu_in=1, batch=3),
    dict(ksplit=8, batch=3),
    dict(colpart=CP),
    dict(colpart=CP, bias=(BIAS, 7), res=(RES, 512, 3000), batch=3),
])
def test_gemm_nt_emits_the_signature(calls, kw):
    gemm.gemm_nt(H.PREC_BF16, EPI_RESIDUAL, **NT, **kw)
    (name, args), = calls
    assert name == ("nppc_gemm_nt_colsum" if "colpart" in kw else "nppc_gemm_nt")
    _check_kinds(name, args)


@pytest.mark.parametrize("kw", [dict(slope=(SLOPE, 7)), dict(stats=(STATS, 4)), dict(relu_in=1), dict(ksplit=2)])
def test_gemm_nt_colpart_excludes_what_the_colsum_entry_lacks(calls, kw):
    with pytest.raises(ValueError):
        gemm.gemm_nt(H.PREC_BF16, EPI_RESIDUAL, **NT, colpart=CP, **kw)
    assert calls == []


def test_gemm_nt_gn_and_reductions_emit_their_signatures(calls):
    gemm.gemm_nt_gn(H.PREC_BF16, A=(A, 512, 1000), B=(B, 512, 2000), C=(C, 320, 3000), u=U, v=V, uv_stride=320,
                    res=(RES, 320, 3000), stats=(STATS, 4), count=float(512 * 101), eps=1e-8, R=256, N=320, K=512, Tp=128, Tv=101,
                    Nv=257, batch=3, stream=S)
    gemm.reduce_slabs(A, 8, slab_stride=1000, ld=64, dst=DST, dst_ld=34, rows=1536, ncols=34, stream=S)
    gemm.reduce_slabs(A, 8, slab_stride=1000, ld=64, dst=DST, dst_ld=1, rows=1536, col0=34, ncols=1, permH=384, accumulate=1,
                      batch=3, s_slab=8000, s_dst=99, stream=S)
    gemm.reduce_slabs_t(A, 8, slab_stride=1000, ld=64, dst=DST, dst_ld=384, rows=10, ncols=384, stream=S)
    assert [n for n, _ in calls] == ["nppc_gemm_nt_gn", "nppc_reduce_slabs", "nppc_reduce_slabs", "nppc_reduce_slabs_t"]
    for name, args in calls:
        _check_kinds(name, args)
    assert calls[0][1] == [H.PREC_BF16, A, 512, 1000, B, 512, 2000, C, 320, 3000, U, V, 320, RES, 320, 3000, STATS, 4,
                           float(512 * 101), 1e-8, 256, 320, 512, 128, 101, 257, 3, S]
    assert calls[1][1] == [A, 8, 1000, 64, DST, 34, 1536, 0, 34, 0, 0, 0, 0, 1, S]
    assert calls[2][1] == [A, 8, 1000, 64, DST, 1, 1536, 34, 1, 384, 1, 8000, 99, 3, S]
    assert calls[3][1] == [A, 8, 1000, 64, DST, 384, 10, 384, 0, 0, 1, S]


# the sizes of a small direction net: C = 6 * 33 -> ldC 256, F = 33 -> ldF 64, B = 4, Tp = 128
prec, Bn, Tp, Tv, Cc, ldC, sP = H.PREC_BF16, 4, 128, 101, 198, 256, 123456
R, sAct = Bn * Tp, Bn * Tp * TCN_HIDDEN


def test_forward_conv1x1_site(calls):
    """FSNEngine.forward, TCN block conv1x1 (EPI_PRELU_STATS): the positional list of the launch before the wrappers"""
    Xin, W1p, y1, st1 = _T("Xin"), _T("W1p[i]"), _T("y1"), _T("st1")
    gemm.gemm_nt(prec, EPI_PRELU_STATS, A=(Xin, ldC, R * ldC), B=(W1p, ldC, TCN_HIDDEN * ldC), C=(y1, TCN_HIDDEN, sAct),
                 bias=(BIAS, sP), slope=(SLOPE, sP), stats=(st1, Bn * 2),
                 R=R, N=TCN_HIDDEN, K=ldC, Tp=Tp, Tv=Tv, Nv=TCN_HIDDEN, batch=3, stream=S)
    assert calls == [("nppc_gemm_nt", [
        prec, EPI_PRELU_STATS, Xin, ldC, R * ldC, W1p, ldC, TCN_HIDDEN * ldC,
        y1, TCN_HIDDEN, sAct, BIAS, sP, None, 0, 0, SLOPE, sP,
        st1, Bn * 2, R, TCN_HIDDEN, ldC, Tp, Tv, TCN_HIDDEN, 0, 3, 1, S])]


def test_backward_residual_colsum_site(calls):
    """FSNEngine backward, conv1x1 input gradient + residual (EPI_RESIDUAL) leaving block i-1's column sums"""
    h2b, W1T, dXi, dXo = _T("h2b"), _T("W1T[i]"), _T("dXi"), _T("dXo")
    gemm.gemm_nt(prec, EPI_RESIDUAL, A=(h2b, TCN_HIDDEN, sAct), B=(W1T, TCN_HIDDEN, ldC * TCN_HIDDEN), C=(dXi, ldC, R * ldC),
                 res=(dXo, ldC, R * ldC), R=R, N=ldC, K=TCN_HIDDEN, Tp=Tp, Tv=Tv, Nv=Cc, batch=3, colpart=CP, stream=S)
    assert calls == [("nppc_gemm_nt_colsum", [
        prec, EPI_RESIDUAL, h2b, TCN_HIDDEN, sAct, W1T, TCN_HIDDEN, ldC * TCN_HIDDEN,
        dXi, ldC, R * ldC, None, 0, dXo, ldC, R * ldC, R, ldC, TCN_HIDDEN, Tp, Tv, Cc, 3, CP, S])]
    calls.clear()
    # the sites that pass `colpart=` emit the plain entry point when there are no column sums to leave (fp32 parity mode, block 0)
    gemm.gemm_nt(prec, EPI_MASK_POS, A=(h2b, TCN_HIDDEN, sAct), B=(W1T, TCN_HIDDEN, ldC * TCN_HIDDEN), C=(dXi, ldC, R * ldC),
                 res=(dXo, ldC, R * ldC), R=R, N=ldC, K=TCN_HIDDEN, Tp=Tp, Tv=Tv, Nv=Cc, batch=3, colpart=None, stream=S)
    assert calls == [("nppc_gemm_nt", [
        prec, EPI_MASK_POS, h2b, TCN_HIDDEN, sAct, W1T, TCN_HIDDEN, ldC * TCN_HIDDEN, dXi, ldC,
        R * ldC, None, 0, dXo, ldC, R * ldC, None, 0, None, 0, R, ldC, TCN_HIDDEN, Tp, Tv, Cc, 0, 3, 1, S])]


def test_wgrad_split_k_site(calls):
    """FSNEngine._wgrad, the batched NT product into split-K fp32 slabs (EPI_PLAIN_F32, batch = 3)"""
    AT, BT, slab = _T("tA"), _T("tB"), _T("slab")
    lda = ldb = R
    sA, sB, rows, ncolsN, K, Sk = 512 * R, 512 * R, 256, TCN_HIDDEN, R, 8
    gemm.gemm_nt(prec, EPI_PLAIN_F32, A=(AT, lda, sA), B=(BT, ldb, sB), C=(slab, ncolsN, rows * ncolsN), R=rows,
                 N=ncolsN, K=K, Tp=rows, Tv=rows, Nv=ncolsN, batch=3, ksplit=Sk, stream=S)
    assert calls == [("nppc_gemm_nt", [
        prec, EPI_PLAIN_F32, AT, lda, sA, BT, ldb, sB, slab, ncolsN, rows * ncolsN, None,
        0, None, 0, 0, None, 0, None, 0, rows, ncolsN, K, rows, rows, ncolsN, 0, 3, Sk, S])]


def test_unet_conv_fwd_sites(calls):
    """UNetEngine: the forward (plain and with the folded BatchNorm) and the input gradient, which swaps the roles of the pack's
    two widths"""
    X, Wf, Wb, Y, DX, SC, SH = (_T(n) for n in "x wf wb y dx scale shift".split())
    geo = dict(B=2, hw=(17, 33), ks=3, stream=S)
    UE.conv_fwd(prec, A=UE._View(X, 128), Wp=Wf, C=UE._View(Y, 256), bias=BIAS, Cin=128, Cout=200, Np=256, **geo)
    UE.conv_fwd(prec, A=UE._View(X, 128), Wp=Wf, C=UE._View(Y, 256), bias=BIAS, fold=(SC, SH), Cin=128, Cout=200, Np=256, **geo)
    UE.conv_fwd(prec, A=UE._View(Y, 256), Wp=Wb, C=UE._View(DX, 128), Cin=256, Cout=128, Np=128, **geo)
    for name, args in calls:
        _check_kinds(name, args)
    assert calls == [
        ("nppc_conv_fwd", [prec, X, 128, Wf, Y, 256, BIAS, None, None, UE.LEAK, 2, 17, 33, 128, 200, 256, 3, S]),
        ("nppc_conv_fwd", [prec, X, 128, Wf, Y, 256, BIAS, SC, SH, UE.LEAK, 2, 17, 33, 128, 200, 256, 3, S]),
        ("nppc_conv_fwd", [prec, Y, 256, Wb, DX, 128, None, None, None, UE.LEAK, 2, 17, 33, 256, 128, 128, 3, S])]


def test_unet_bn_bwd_sites(calls):
    """UNetEngine._double_conv_bwd: one gradient, two gradients (decoder + skip), and the block that ends in nn.Dropout"""
    DA, DB, Y, X, SS, ST, DX, DG, DBETA = (_T(n) for n in "dyA dyB y x ss st dx dgamma dbeta".split())
    kw = dict(dyA=UE._View(DA, 512), Y=UE._View(Y, 1024), X=UE._View(X, 512), ss=SS, S=ST, dX=UE._View(DX, 512), dgamma=DG,
              dbeta=DBETA, C=512, B=2, hw=(4, 8), stream=S)
    UE.bn_bwd(prec, **kw)
    UE.bn_bwd(prec, dyB=UE._View(DB, 1024), **kw)
    UE.bn_bwd(prec, dyB=UE._View(DB, 1024), drop=(0.2, 5, 29), **kw)
    for name, args in calls:
        _check_kinds(name, args)
    tail = [Y, 1024, X, 512, SS, ST, DX, 512, DG, DBETA, 512, 2, 4, 8, UE.LEAK]
    assert calls == [("nppc_bn_bwd", [prec, DA, 512, None, 0] + tail + [S]),
                     ("nppc_bn_bwd", [prec, DA, 512, DB, 1024] + tail + [S]),
                     ("nppc_bn_bwd_dropout", [prec, DA, 512, DB, 1024] + tail + [0.2, 5, 29, S])]


@pytest.mark.parametrize("case, args, expect", [
    # FullSubNet+ defaults (sb hidden 384, 15 neighbours: I = 34 staged as KX = 64), bf16, guard rows kept by the train forward
    ("c2: 32 x 4 s, T' = 251 + 2", (H.PREC_BF16, 384, 64, 253, 64, True), ("fused2", True)),
    ("c3: the same net and clips", (H.PREC_BF16, 384, 64, 253, 64, True), ("fused2", True)),
    ("c5: 8 x 30 s, T' = 1876 + 2", (H.PREC_BF16, 384, 64, 1878, 64, True), ("fused2", True)),
    # 4H = 1024: fold_bias holds (4 * 2 * 64 = 512 workgroups), 256 is no multiple of 192
    ("H = 256", (H.PREC_BF16, 256, 64, 253, 64, True), ("tn", True)),
    # 4H = 1280, 320 % 128 != 0: no fold either
    ("H = 320", (H.PREC_BF16, 320, 64, 253, 64, True), ("tn", False)),
    ("KX = 128", (H.PREC_BF16, 384, 128, 253, 64, True), ("tn", True)),
    ("one step: no h_{t-1} products", (H.PREC_BF16, 384, 64, 1, 64, True), ("tn", True)),
    ("no guard rows", (H.PREC_BF16, 384, 64, 253, 64, False), ("tn", True)),
    # (4H / 256) * (H / 128) * S = 6 * 3 * 8 = 144 < 256 workgroups: too few K-slices to fold
    ("8 K-slices", (H.PREC_BF16, 384, 64, 253, 8, True), ("tn", False)),
    ("H = 96: 4H % 128 == 0, H % 64 != 0", (H.PREC_BF16, 96, 64, 253, 64, True), ("generic", False)),
    ("fp32", (H.PREC_F32, 384, 64, 253, 64, True), ("generic", False)),
])
def test_lstm_wgrad_mode(case, args, expect):
    assert WGRAD_SPLITS == 64
    assert gemm.lstm_wgrad_mode(*args) == expect, case
