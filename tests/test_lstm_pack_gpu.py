"""The three packings of the cooperative LSTM backward weights (csrc/lstm_coop.hip: nppc_lstm2_coop_bwd_pack, _bwd2_pack,
_bwd4_pack) compared element for element with a NumPy restatement of their layouts.

Every packed buffer is [cu][wave 12][kk][slot][lane l 64][j 8] bf16, one MFMA B fragment per (cu, wave, kk, slot):
    k = 32 kk + 8 (l >> 4) + j = ul * 4 + g',  g' in (i, g, f, o) -> torch gate block (0, 2, 1, 3)[g'],  n = l & 15
    weight row = block * H + unit,  value = W[row][column]  (W_ih columns >= I and unused slots are zero)
  output split (2 CUs, 48 k-steps, 2 slots): unit = ul over ALL units;  u = 192 cu + 16 wave + n
    layer 2: slot 0 -> W_ih[row][u], slot 1 -> W_hh[row][u]
    layer 1: slot 0 -> W_hh[row][u], slot 1 -> W_ih[row][32 cu + 16 wave + n] for wave < 2, else 0
  K-split on CU pairs (2 CUs, 24 k-steps, 4 slots): unit = 192 cu + ul;  c = 16 (wave + 12 slot) + n
    layer 2: c < 384 -> W_ih[row][c], else W_hh[row][c - 384]
    layer 1: c < 384 -> W_hh[row][c];  384 <= c < 448 -> W_ih[row][c - 384];  else 0
  K-split on four-CU clusters (4 CUs, 12 k-steps, 4 slots = owner O): unit = 96 cu + ul
    layer 2: wave < 6 -> W_ih[row][96 O + 16 wave + n], else W_hh[row][96 O + 16 (wave - 6) + n]
    layer 1: wave < 6 -> W_hh[row][96 O + 16 wave + n];  wave == 6 -> W_ih[row][16 O + n];  wave > 6 -> 0
The weights are random bf16-exact values, so the packed bf16 must equal the source bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 384
ZERO, IH, HH = 0, 1, 2


def _columns(layout, layer, cu, wave, slot, n):
    """(matrix, column) of every element, broadcast over the index grids"""
    if layout == "osplit":
        u = 192 * cu + 16 * wave + n + 0 * slot
        if layer == 2:
            return np.where(slot == 0, IH, HH) + 0 * u, u
        return np.where(slot == 0, HH, np.where(wave < 2, IH, ZERO)) + 0 * u, np.where(slot == 0, u, 32 * cu + 16 * wave + n)
    if layout == "ksplit2":
        c = 16 * (wave + 12 * slot) + n + 0 * cu
        if layer == 2:
            return np.where(c < HD, IH, HH), np.where(c < HD, c, c - HD)
        return np.where(c < HD, HH, np.where(c < HD + 64, IH, ZERO)), np.where(c < HD, c, c - HD)
    assert layout == "ksplit4"
    owner = slot
    if layer == 2:
        return np.where(wave < 6, IH, HH) + 0 * (owner + n + cu), 96 * owner + 16 * (wave % 6) + n + 0 * cu
    return (np.where(wave < 6, HH, np.where(wave == 6, IH, ZERO)) + 0 * (owner + n + cu),
            np.where(wave < 6, 96 * owner + 16 * wave + n, 16 * owner + n) + 0 * cu)


GEOM = {"osplit": (2, 48, 2, 0), "ksplit2": (2, 24, 4, 192), "ksplit4": (4, 12, 4, 96)}   # CUs, k-steps, slots, units per CU


def _expected(layout, layer, w_ih, w_hh):
    G, nkk, slots, upc = GEOM[layout]
    cu, wave, kk, slot, l, j = np.meshgrid(np.arange(G), np.arange(12), np.arange(nkk), np.arange(slots), np.arange(64),
                                           np.arange(8), indexing="ij", sparse=True)
    k = 32 * kk + 8 * (l >> 4) + j
    row = np.array([0, 2, 1, 3])[k & 3] * HD + upc * cu + (k >> 2)
    mat, col = _columns(layout, layer, cu, wave, slot, l & 15)
    shape = np.broadcast_shapes(row.shape, mat.shape, col.shape)
    row, mat, col = (np.broadcast_to(a, shape) for a in (row, mat, col))
    I = w_ih.shape[1]
    v_ih = np.where(col < I, w_ih[row, np.minimum(col, I - 1)], np.float32(0))
    v_hh = w_hh[row, np.minimum(col, HD - 1)]
    return np.where(mat == HH, v_hh, np.where(mat == IH, v_ih, np.float32(0))).astype(np.float32).reshape(-1)


def _bf16_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("I", [34, 64])
def test_backward_weight_packings_match_layouts(I):
    from nppc_audio import _hip as H
    g = torch.Generator().manual_seed(7 + I)
    src = [(torch.randn(4 * HD, c, generator=g) * 0.1).bfloat16().float() for c in (I, HD, HD, HD)]   # w_ih0, w_hh0, w_ih1, w_hh1
    dev = torch.device("cuda")
    ws = [t.to(dev) for t in src]
    w = [t.numpy() for t in src]
    n = ctypes.c_long()
    sizes = {}
    H.call("nppc_lstm2_coop_bwd_packed_elems", ctypes.byref(n))
    sizes["osplit"] = n.value
    H.call("nppc_lstm2_coop_bwd2_packed_elems", ctypes.byref(n))
    sizes["ksplit2"] = n.value
    nx, nf = ctypes.c_long(), ctypes.c_long()
    H.call("nppc_lstm2_coop_bwd4_sizes", 64, ctypes.byref(n), ctypes.byref(nx), ctypes.byref(nf))
    sizes["ksplit4"] = n.value
    fns = {"osplit": "nppc_lstm2_coop_bwd_pack", "ksplit2": "nppc_lstm2_coop_bwd2_pack", "ksplit4": "nppc_lstm2_coop_bwd4_pack"}
    for layout, fn in fns.items():
        G, nkk, slots, _ = GEOM[layout]
        assert sizes[layout] == G * 12 * nkk * slots * 512
        # poisoned: every element must be written
        wb1 = torch.full((sizes[layout],), float("nan"), dtype=torch.bfloat16, device=dev)
        wb2 = torch.full((sizes[layout],), float("nan"), dtype=torch.bfloat16, device=dev)
        H.call(fn, *ws, I, wb1, wb2, H.stream())
        torch.cuda.synchronize()
        for layer, wb, w_ih, w_hh in ((1, wb1, w[0], w[1]), (2, wb2, w[2], w[3])):
            want = _expected(layout, layer, w_ih, w_hh)
            want_bits = (want.view(np.uint32) >> 16).astype(np.uint16)
            assert ((want_bits.astype(np.uint32) << 16).view(np.float32) == want).all()      # the references are bf16-exact
            got = _bf16_bits(wb)
            bad = np.flatnonzero(got != want_bits)
            assert bad.size == 0, (layout, layer, I, bad.size, bad[:8].tolist())
