"""Enhance a whole noisy recording: chunk, run the nets, align the directions, splice, on the device (csrc/enhance_core.h,
csrc/enhance_rec.hip; specification tests/enhance_ref.py).

Every other entry point of the speech-enhancement side takes clips that are already cut.  `RecordingEnhancer.enhance` takes
the recording itself:

    plan_chunks -> [n, C] chunks at a hop of H = C / 2 -> ragged STFT, restorer, K-head direction net (NPPCModel, in batches
    of chunk_batch) -> K + 1 inverse STFTs per chunk in one ragged launch -> boundary Gram -> chain -> splice

and returns the enhanced recording and, with `alphas`, the K x A recordings `enhanced + alpha PC_k`.  The chunking is the
reference's Inferencer.overlapped_chunk (fullsubnet_plus/inferencer/inferencer.py:192-250): Hann-weighted chunks at 50 %
overlap, the first half of the first chunk unweighted; here the last chunk's tail is unweighted too.  The reference has
nothing for the directions.

Why the directions need the two steps in the middle: a principal direction is defined up to sign, and two directions of close
variance can change places from one chunk to the next.  Cross-fading `e + alpha p_k` of chunk c - 1 into that of chunk c then
cancels the variation where the sign flipped and blends unrelated directions where the order changed.  So for every boundary
the K x K cosines between the directions of the two chunks over their shared H samples are formed (nppc_enh_gram), a serial
greedy walk matches and sign-aligns chunk c to chunk c - 1 (nppc_enh_chain), and the splice reads the resulting tables from
device memory (nppc_enh_splice).  The host never sees them unless the caller reads the returned tensors.

`enhance(..., samples=S)` also draws S posterior samples of the whole recording (the rule: item 4 of
csrc/enhance_core.h; csrc/enhance_post.hip; specification tests/enhance_posterior_ref.py): ONE set of coefficients z [S, K]
per recording, indexed by slot, which the alignment tables carry from chunk to chunk; `sample_chunks` builds every chunk's
sampled mask in slot order, inverts and cross-fades in one launch, with no [n, S, C] intermediate.

A spliced direction is NOT a principal direction of the whole recording's posterior: it is a chain of per-chunk directions,
each the nearest one of the next chunk.  'continuity' says how near: where it is small the spliced variation means little.
"""
import ctypes
import functools
import os
from typing import Literal

import pydantic
import torch

from . import _hip as H
from . import ops
from .nppc_model import NPPCModel, NPPCModelConfig

__all__ = ["RecordingEnhancerConfig", "RecordingEnhancer", "plan_chunks", "splice_chunks", "hann_table", "enh_shape",
           "boundary_gram", "chain", "splice", "chain_host", "splice_host", "enh_post_shape", "check_sample_chunk_args",
           "sample_chunks", "MAX_K", "MAX_SPLIT", "MATCH"]

MAX_K = 16                   # NPPC_ENH_MAX_K
MAX_SPLIT = 64               # NPPC_ENH_MAX_SPLIT
MATCH = {"greedy": 0, "sign": 1}


class RecordingEnhancerConfig(pydantic.BaseModel):
    model_configuration: NPPCModelConfig
    checkpoint_path: str                       # NPPCAudioTrainer.save_checkpoint's file (NPPCAudioValidator's)
    device: str = "cuda"
    sample_rate: int = 16000
    chunk_samples: int = 65536                 # C; adjacent chunks overlap by C / 2
    chunk_batch: int = 32                      # chunks per forward
    match: Literal["greedy", "sign"] = "greedy"


def plan_chunks(length, chunk_samples, n_fft, hop_length, kersize):
    """The chunks of a recording of `length` samples: [(start, length)], ascending.  With C = chunk_samples, H = C // 2:
    one chunk (0, L) when L <= C, else ceil((L - C) / H) + 1 chunks, chunk c from c H with min(C, L - c H) samples: every
    chunk but the last has C samples, the last more than H, and adjacent chunks share exactly H.
    ValueError for an odd or non-positive C, for H < hop_length max(kersize) or H < n_fft // 2 (the ragged forward could
    refuse a last chunk), and for a recording the ragged forward refuses (ops.ragged_lengths, fullsubnet.check_frames).
    No GPU."""
    L, C, hop, n_fft = int(length), int(chunk_samples), int(hop_length), int(n_fft)
    kmax = max(int(k) for k in kersize)
    if C <= 0 or C % 2:
        raise ValueError(f"chunk_samples = {C}: a positive even number of samples")
    Hh = C // 2
    if hop <= 0 or n_fft < 2:
        raise ValueError(f"n_fft {n_fft}, hop_length {hop}: not an STFT configuration")
    if Hh < hop * kmax or Hh < n_fft // 2:
        raise ValueError(f"chunk_samples = {C}: half a chunk ({Hh} samples) is shorter than hop_length x the largest TSSE "
                         f"kernel ({hop} x {kmax}) or than n_fft // 2 ({n_fft // 2})")
    if L <= n_fft // 2 or 1 + L // hop < kmax:
        raise ValueError(f"the recording has {L} samples: it needs more than n_fft // 2 = {n_fft // 2} and at least {kmax} "
                         f"frames of {hop}")
    if L <= C:
        return [(0, L)]
    n = -(-(L - C) // Hh) + 1
    return [(c * Hh, min(C, L - c * Hh)) for c in range(n)]


@functools.lru_cache(maxsize=8)
def _hann_table(C, device):
    import numpy as np
    w = torch.from_numpy((0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(C // 2, dtype=np.float64) / C)).astype(np.float32))
    return w if device is None else w.to(device)


def hann_table(chunk_samples, device=None):
    """w[i] = 0.5 - 0.5 cos(2 pi i / C), i < C // 2: fp64 on the host, rounded to fp32 (no device cosine enters the splice).
    Made once per (C, device) and shared: do not write to it."""
    return _hann_table(int(chunk_samples), None if device is None else str(torch.device(device)))


def enh_shape(n, K, chunk_samples, split=0):
    """nppc_enh_shape -> (S, workspace bytes).  No GPU."""
    S, nbytes = ctypes.c_int(), ctypes.c_long()
    H.call("nppc_enh_shape", int(n), int(K), int(chunk_samples), int(split), ctypes.byref(S), ctypes.byref(nbytes))
    return S.value, nbytes.value


def _rows(t):
    """a float32 tensor whose last dimension is contiguous, as it is when it can be (strided views of one buffer stay)"""
    if t.dtype != torch.float32 or t.stride(-1) != 1 or any(s < 0 for s in t.stride()):
        t = t.float().contiguous()
    return t


def _check_chunks(enh, pcs):
    if enh.dim() != 2 or pcs.dim() != 3 or pcs.shape[0] != enh.shape[0] or pcs.shape[2] != enh.shape[1]:
        raise ValueError(f"chunks {tuple(enh.shape)} and directions {tuple(pcs.shape)}: want [n, C] and [n, K, C]")
    n, K, C = pcs.shape
    if n < 1 or C < 2 or C % 2:
        raise ValueError(f"{n} chunks of {C} samples: want at least one chunk of an even length")
    if K > MAX_K:
        raise ValueError(f"{K} directions: at most {MAX_K}")
    return n, K, C


def _check_last(n, C, last_length):
    last = int(last_length)
    if not (0 < last <= C) or (n > 1 and last <= C // 2):
        raise ValueError(f"last_length = {last}: the last of {n} chunks of {C} has 1 .. {C} samples, and more than {C // 2} "
                         "when it is not the only one")
    return (n - 1) * (C // 2) + last


def boundary_gram(pcs, split=0):
    """nppc_enh_gram: pcs [n, K, C] (device, n >= 2, K >= 1) -> (work [n - 1, S, K (K + 2)] fp64, S)"""
    H.require_gpu()
    pcs = _rows(pcs)
    n, K, C = pcs.shape
    S, _ = enh_shape(n, K, C, split)
    work = torch.empty(n - 1, S, K * (K + 2), dtype=torch.float64, device=pcs.device)
    H.call("nppc_enh_gram", H.c_p(pcs.data_ptr()), pcs.stride(0), pcs.stride(1), n, K, C, S, work, H.stream())
    return work, S


def chain(work, n, K, match="greedy", want_gram=False, device=None):
    """nppc_enh_chain: boundary_gram's work (None for n = 1) -> (perm [n, K] int32, sign [n, K] int32, continuity [n - 1, K]
    fp64) and, with want_gram, the summed gram [n - 1, K (K + 2)] fp64"""
    H.require_gpu()
    if n > 1 and (work is None or work.dim() != 3 or work.shape[0] != n - 1 or work.shape[2] != K * (K + 2)
                  or work.dtype != torch.float64 or not work.is_contiguous()):
        raise ValueError(f"work {None if work is None else tuple(work.shape)}: want boundary_gram's [{n - 1}, S, {K * (K + 2)}] fp64")
    dev = work.device if work is not None else device
    perm = torch.empty(n, K, dtype=torch.int32, device=dev)
    sign = torch.empty_like(perm)
    cont = torch.empty(n - 1, K, dtype=torch.float64, device=dev)
    gram = torch.empty(n - 1, K * (K + 2), dtype=torch.float64, device=dev)
    S = work.shape[1] if work is not None else 1
    H.call("nppc_enh_chain", work if n > 1 else None, n, K, S, MATCH[match], perm, sign, cont if n > 1 else None,
           gram if n > 1 else None, H.stream())
    return (perm, sign, cont, gram) if want_gram else (perm, sign, cont)


def _alphas(alphas, device):
    if alphas is None:
        return None
    if isinstance(alphas, torch.Tensor):
        return alphas.reshape(-1).to(device=device, dtype=torch.float32).contiguous()
    return torch.tensor([float(a) for a in alphas], dtype=torch.float32).to(device)


def splice(enh, pcs, last_length, alphas, perm, sign, w=None):
    """nppc_enh_splice: enh [n, C], pcs [n, K, C] (or None), alphas [A] (or None), perm / sign [n, K] int32 device tables
    -> [1 + K A, L] (a view of rows padded to a multiple of four samples): row 0 the enhanced recording, row 1 + s A + a
    slot s at alphas[a]"""
    H.require_gpu()
    enh = _rows(enh)
    a = _alphas(alphas, enh.device)
    A = 0 if a is None or pcs is None else a.numel()
    if A:
        pcs = _rows(pcs)
        n, K, C = _check_chunks(enh, pcs)
        if tuple(perm.shape) != (n, K) or tuple(sign.shape) != (n, K):
            raise ValueError(f"perm {tuple(perm.shape)}, sign {tuple(sign.shape)}: want [{n}, {K}]")
        perm, sign = perm.to(enh.device, torch.int32).contiguous(), sign.to(enh.device, torch.int32).contiguous()
        pp, pcs_s = H.c_p(pcs.data_ptr()), (pcs.stride(0), pcs.stride(1))
    else:
        (n, C), K = enh.shape, 0
        if C < 2 or C % 2:
            raise ValueError(f"chunks of {C} samples: want an even length")
        perm = sign = a = None
        pp, pcs_s = H.c_p(0), (0, 0)
    L = _check_last(n, C, last_length)
    if w is None and n > 1:
        w = hann_table(C, enh.device)
    ldo = (L + 3) // 4 * 4
    out = torch.empty(1 + K * A, ldo, dtype=torch.float32, device=enh.device)
    H.call("nppc_enh_splice", H.c_p(enh.data_ptr()), enh.stride(0), pp, pcs_s[0], pcs_s[1], n, K, C, L, a, A, w, perm, sign, out,
           ldo, H.stream())
    return out[:, :L]


def splice_chunks(enh, pcs, last_length, alphas=None, match="greedy", split=0):
    """The device steps of `enhance` on chunk waveforms the caller supplies: enh [n, C] (e_c), pcs [n, K, C] (p_{c,k}), the
    last chunk holding last_length samples -> dict: 'enhanced' [L]; with alphas [A] also 'variations' [K, A, L], 'perm'
    [n, K] int32, 'sign' [n, K] int32, 'continuity' [n - 1, K] fp64 (|cosine| of each spliced direction across each
    boundary).  Strided views of one buffer are taken as they are.  No host read."""
    if match not in MATCH:
        raise ValueError(f"match = {match!r}: 'greedy' or 'sign'")
    n, K, C = _check_chunks(enh, pcs)
    _check_last(n, C, last_length)                                              # before any launch
    if alphas is None or K == 0:
        return {"enhanced": splice(enh, None, last_length, None, None, None)[0]}
    work = boundary_gram(pcs, split)[0] if n > 1 else None
    perm, sign, cont = chain(work, n, K, match, device=enh.device)
    a = _alphas(alphas, enh.device)
    full = splice(enh, pcs, last_length, a, perm, sign)
    return {"enhanced": full[0], "variations": full[1:].unflatten(0, (K, a.numel())), "perm": perm, "sign": sign,
            "continuity": cont}


def chain_host(pcs, match="greedy", want_gram=False):
    """nppc_enh_chain_host: pcs [n, K, C] on the host -> (perm, sign, continuity[, gram]) as `chain` returns them.  No GPU."""
    pcs = pcs.float().contiguous()
    n, K, C = pcs.shape
    perm = torch.empty(n, K, dtype=torch.int32)
    sign = torch.empty_like(perm)
    cont = torch.empty(n - 1, K, dtype=torch.float64)
    gram = torch.empty(n - 1, K * (K + 2), dtype=torch.float64)
    p = lambda t: H.c_p(t.data_ptr() if t.numel() else 0)                              # noqa: E731
    H.call("nppc_enh_chain_host", p(pcs), pcs.stride(0), pcs.stride(1), n, K, C, MATCH[match], p(perm), p(sign),
           p(cont) if n > 1 else H.c_p(0), p(gram) if n > 1 else H.c_p(0))
    return (perm, sign, cont, gram) if want_gram else (perm, sign, cont)


def splice_host(enh, pcs, last_length, alphas, perm, sign):
    """nppc_enh_splice_host: `splice` on host tensors, the same core run serially.  No GPU."""
    enh = enh.float().contiguous()
    n, C = enh.shape
    a = None if alphas is None else torch.as_tensor(alphas, dtype=torch.float32).reshape(-1).contiguous()
    A = 0 if a is None or pcs is None else a.numel()
    K = pcs.shape[1] if A else 0
    L = _check_last(n, C, last_length)
    w = hann_table(C)
    out = torch.empty(1 + K * A, L, dtype=torch.float32)
    p = lambda t: H.c_p(t.data_ptr() if t is not None and t.numel() else 0)           # noqa: E731
    if A:
        pcs = pcs.float().contiguous()
        perm, sign = perm.to(torch.int32).contiguous(), sign.to(torch.int32).contiguous()
        strides = (pcs.stride(0), pcs.stride(1))
    else:
        pcs = perm = sign = a = None
        strides = (0, 0)
    H.call("nppc_enh_splice_host", p(enh), enh.stride(0), p(pcs), strides[0], strides[1], n, K, C, L, p(a), A, p(w), p(perm),
           p(sign), p(out), L)
    return out


def enh_post_shape(n, S, K, chunk_samples, length, T, nfft, hop, stats=False):
    """nppc_enh_post_sample_shape -> (sample tiles, samples per tile, workspace bytes); ValueError for what the kernel does
    not take.  No GPU."""
    tiles, per, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    try:
        H.call("nppc_enh_post_sample_shape", int(n), int(S), int(K), int(chunk_samples), int(length), int(T), int(nfft), int(hop),
               1 if stats else 0, ctypes.byref(tiles), ctypes.byref(per), ctypes.byref(nbytes))
    except RuntimeError as e:
        raise ValueError(f"recording posterior: n {n}, S {S}, K {K}, chunk_samples {chunk_samples}, length {length}, T {T}, "
                         f"n_fft {nfft}, hop {hop}: {e}") from e
    return tiles.value, per.value, nbytes.value


def check_sample_chunk_args(pred_shape, w_shape, re_shape, im_shape, lengths, z_shape, perm_shape, sign_shape, last_length,
                            chunk_samples, nfft, hop, domain, samples, stats):
    """every refusal of sample_chunks as a ValueError, from shapes alone (no GPU, no launch) -> (n, S, K, F, T, L)"""
    from .posterior import DOMAINS, MAX_STAT_S, config_ok
    C, nfft, hop = int(chunk_samples), int(nfft), int(hop)
    if not config_ok(nfft, hop) or nfft // hop < 2:
        raise ValueError(f"recording posterior: n_fft {nfft} / hop {hop} outside n_fft in (64, 128, 256, 512), n_fft % hop == 0, "
                         "2 <= n_fft / hop <= 8")
    if C <= 0 or C % 2 or (C // 2) % (4 * hop):
        raise ValueError(f"chunk_samples = {C}: half a chunk has to be a multiple of 4 hop = {4 * hop} samples")
    if domain not in DOMAINS:
        raise ValueError(f"domain must be one of {sorted(DOMAINS)}, got {domain!r}")
    if not (samples or stats):
        raise ValueError("recording posterior: nothing asked for (samples and stats are both off)")
    F = nfft // 2 + 1
    if len(pred_shape) != 4 or pred_shape[0] < 1 or pred_shape[1] != 2 or pred_shape[2] != F:
        raise ValueError(f"pred_crm is [n,2,{F},T], got {tuple(pred_shape)}")
    n, _, _, T = pred_shape
    if len(w_shape) != 5 or tuple(w_shape[:1]) + tuple(w_shape[2:]) != (n, 2, F, T):
        raise ValueError(f"w_mat is [n,K,2,F,T] = [{n},K,2,{F},{T}], got {tuple(w_shape)}")
    K = w_shape[1]
    if K > MAX_K:
        raise ValueError(f"{K} directions: at most {MAX_K}")
    if tuple(re_shape) != (n, F, T) or tuple(im_shape) != (n, F, T):
        raise ValueError(f"the noisy planes are [{n},{F},{T}], got {tuple(re_shape)} and {tuple(im_shape)}")
    if len(z_shape) != 3 or z_shape[0] < 1 or z_shape[1] != K or z_shape[2] != 2:
        raise ValueError(f"coefficients are [S,{K}], one set per recording, got {tuple(z_shape[:2])}")
    S = z_shape[0]
    if stats and not 2 <= S <= MAX_STAT_S:
        raise ValueError(f"statistics need 2 <= S <= {MAX_STAT_S} samples, got {S}")
    if tuple(perm_shape) != (n, K) or tuple(sign_shape) != (n, K):
        raise ValueError(f"perm {tuple(perm_shape)}, sign {tuple(sign_shape)}: want [{n}, {K}]")
    L = _check_last(n, C, last_length)
    want = [C] * (n - 1) + [int(last_length)]
    if lengths is not None:
        host = [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
        if host != want:
            raise ValueError(f"lengths {host}: the chunks of this plan have {want} samples")
    if int(last_length) <= nfft // 2:
        raise ValueError(f"last_length = {int(last_length)} is too short (needs more than {nfft // 2} samples)")
    if ops.stft_frames(max(want), hop) > T:
        raise ValueError(f"a chunk of {max(want)} samples needs {ops.stft_frames(max(want), hop)} frames, the planes have {T}")
    return n, S, K, F, T, L


def sample_chunks(pred_crm, w_mat, re, im, lengths, coeffs, perm, sign, last_length, chunk_samples, nfft, hop,
                  domain="compressed", samples=True, stats=False):
    """nppc_enh_post_sample: posterior samples of a whole recording from the planes of its chunks, in one launch.

    pred_crm [n,2,F,T] compressed, w_mat [n,K,2,F,T], noisy re / im [n,F,T] (or [n,1,F,T]) of the n chunks of plan_chunks,
    lengths their sample counts (None: chunk_samples each and last_length for the last; anything else is refused), coeffs
    [S,K] real or complex, or [S,K,2]: ONE set per recording, indexed by slot; perm / sign [n,K] the device tables of `chain`.
    Sample s of chunk c is posterior.sample_waveforms' sample with the directions sign[c][k] w_mat[c][perm[c][k]], k
    ascending over the slots; the recording is their cross-fade by `splice`'s rule (hann_table).
    -> dict: "samples" [S,L] (samples=True; a view of rows padded to a multiple of four samples), "mean", "std" [L] over the
    samples (stats=True).  With samples=False nothing of size S L is allocated.  ValueError before any launch for what the
    kernel does not take (check_sample_chunk_args)."""
    from .posterior import DOMAINS, as_coefficients
    if not isinstance(coeffs, torch.Tensor):
        raise ValueError("coeffs is a tensor [S,K] (real or complex) or [S,K,2]")
    z = as_coefficients(coeffs[None])[0]
    if re.dim() == 4:
        re, im = re.squeeze(1), im.squeeze(1)
    n, S, K, F, T, L = check_sample_chunk_args(pred_crm.shape, w_mat.shape, re.shape, im.shape, lengths, z.shape, perm.shape,
                                               sign.shape, last_length, chunk_samples, nfft, hop, domain, samples, stats)
    C = int(chunk_samples)
    _, _, nbytes = enh_post_shape(n, S, K, C, L, T, nfft, hop, stats)
    H.require_gpu()
    pred_crm, w_mat, re, im = (ops._f32c(t) for t in (pred_crm, w_mat, re, im))
    dev = pred_crm.device
    z = z.to(dev).contiguous()
    perm, sign = perm.to(dev, torch.int32).contiguous(), sign.to(dev, torch.int32).contiguous()
    w = hann_table(C, dev) if n > 1 else None
    out = {}
    ldo = (L + 3) // 4 * 4
    rows = torch.empty(S, ldo, dtype=torch.float32, device=dev) if samples else None
    if stats:
        out["mean"], out["std"] = (torch.empty(L, dtype=torch.float32, device=dev) for _ in range(2))
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        H.call("nppc_enh_post_sample", pred_crm, w_mat if K else None, re, im, z if K else None, perm if K else None,
               sign if K else None, w, DOMAINS[domain], n, S, K, C, L, T, int(nfft), int(hop), rows, ldo, out.get("mean"),
               out.get("std"), work, nbytes, H.stream())
    if samples:
        out["samples"] = rows[:, :L]
    return out


class RecordingEnhancer:
    """Loads the checkpoint NPPCAudioValidator loads ({'model_state_dict': ...} of an NPPCModel: frozen restorer and
    direction net) and enhances whole recordings with it."""

    def __init__(self, config: RecordingEnhancerConfig):
        from pathlib import Path
        self.config = config
        self.device = config.device
        if config.device == "cuda":
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        path = Path(config.checkpoint_path).expanduser().absolute()
        if not path.exists():
            raise FileNotFoundError(f"Model file not found: {path}")
        checkpoint = torch.load(path.as_posix(), map_location="cpu")
        self.model = NPPCModel(config.model_configuration)
        self.model.load_state_dict(checkpoint["model_state_dict"])
        self.model.to(self.device)
        self.model.eval()

    def _stft(self):
        st = self.config.model_configuration.stft_configuration
        if st.win_length != st.nfft:
            raise NotImplementedError("win_length == nfft is the STFT configuration built for MI355X")
        return st

    def plan(self, length):
        st = self._stft()
        kersize = list(self.model.pretrained_restoration_model.kersize) + list(self.model.audio_pc_wrapper.net.kersize)
        return plan_chunks(length, self.config.chunk_samples, st.nfft, st.hop_length, kersize)

    def chunk_waveforms(self, x, plan, with_directions=True, keep_planes=False):
        """x [L] (device) and its plan -> buf [n, K + 1, C] (or [n, 1, C]): per chunk the enhanced waveform e_c, then the
        waveform p_{c,k} of ops.crm_directions_to_spectrograms' direction k.  Chunks run through NPPCModel's ragged path
        (lengths=) in batches of chunk_batch, so a chunk's output does not depend on its batch; each batch ends in ONE
        ragged ops.istft launch of its (K + 1) b spectra.  Samples past the last chunk's length are not written.
        keep_planes (with directions): -> (buf, planes), planes = {"pred_crm" [n, 2, F, T], "w_mat" [n, K, 2, F, T], "re",
        "im" [n, F, T]}, what sample_chunks reads: (2 K + 4) F T 4 bytes per chunk on top of buf, about 1.1 GB for a 10 min
        recording at K = 5 and the default chunks (292 chunks of 257 x 257 bins)."""
        c, st = self.config, self._stft()
        n, C = len(plan), c.chunk_samples
        Hh = C // 2
        W = plan[0][1] if n == 1 else C                                         # one chunk keeps the recording's width
        chunks = torch.zeros(n, W, dtype=torch.float32, device=x.device)
        if n == 1:
            chunks[0] = x
        else:
            chunks[:n - 1] = x.unfold(0, C, Hh)[:n - 1]
            chunks[n - 1, :plan[-1][1]] = x[plan[-1][0]:]
        buf = planes = None
        with torch.no_grad():
            for b0 in range(0, n, max(1, c.chunk_batch)):
                xb = chunks[b0:b0 + max(1, c.chunk_batch)]
                lens = [ln for _, ln in plan[b0:b0 + xb.shape[0]]]
                if with_directions:
                    w_mat = self.model(xb, lengths=lens)                        # [b, K, 2, F, T]
                    f = self.model._front(xb, lengths=lens)                     # the memo of the forward above
                else:
                    f = self.model._front(xb, reuse=False, lengths=lens)
                _, re, im = ops.cirm_decompress_apply(f["pred_crm"], f["re"], f["im"])
                re, im = re[:, None], im[:, None]
                if with_directions:
                    d_re, d_im = ops.crm_directions_to_spectrograms(w_mat, f["re"], f["im"])
                    re, im = torch.cat((re, d_re), 1), torch.cat((im, d_im), 1)
                b, V = re.shape[:2]
                waves = ops.istft(re.reshape(b * V, *re.shape[2:]), im.reshape(b * V, *im.shape[2:]), st.nfft, st.hop_length, W,
                                  lengths=[ln for ln in lens for _ in range(V)])
                if buf is None:
                    buf = torch.empty(n, V, C, dtype=torch.float32, device=x.device)
                buf[b0:b0 + b, :, :W] = waves.view(b, V, W)
                if keep_planes and with_directions:
                    kept = {"pred_crm": f["pred_crm"], "w_mat": w_mat, "re": f["re"], "im": f["im"]}
                    if planes is None:
                        planes = {k: torch.empty(n, *t.shape[1:], dtype=torch.float32, device=x.device) for k, t in kept.items()}
                    for k, t in kept.items():
                        planes[k][b0:b0 + b] = t
        return (buf, planes) if keep_planes and with_directions else buf

    def enhance(self, wave, alphas=None, sample_rate=None, samples=0, seed=None, coeffs=None, domain="compressed", temperature=1.0,
                keep_samples=True, stats=False):
        """wave [L] float (host or device) -> dict: 'enhanced' [L]; 'chunks' (plan_chunks' list); with `alphas` [A] also
        'variations' [K, A, L] (enhanced + alpha PC_k, the K directions aligned from chunk to chunk), 'perm' [n, K] int32,
        'sign' [n, K] int32 and 'continuity' [n - 1, K] fp64, device tensors (module docstring).
        The inverse STFT is linear, so e + alpha p IS the variation: K + 1 transforms per chunk serve every alpha.
        No host read beyond what NPPCModel's forward does.
        sample_rate: None or config.sample_rate runs exactly the above.  Another rate: the recording is resampled to
        config.sample_rate (nppc_audio.resample), enhanced there, and every output row is resampled back and cut to L; the
        WHOLE output is then band-limited to config.sample_rate / 2 (unlike restoration, which keeps the input outside its
        gaps, every sample of an enhanced recording comes from the nets).  'chunks' is the plan at the model's rate.

        samples=S > 0 (or coeffs [S, K] real or complex, or [S, K, 2]) also draws S posterior samples of the recording
        (sample_chunks; module docstring): the dict gains 'samples' [S, L] (keep_samples), 'coeffs' [S, K, 2]
        (posterior.draw_coefficients(1, S, K, seed=seed, temperature=temperature)[0] unless given), with stats 'sample_mean'
        and 'sample_std' [L], and 'perm', 'sign', 'continuity', which are formed as above whether or not `alphas` is given.
        keep_samples=False with stats=True allocates nothing of size S L.  Every chunk's planes are then kept until the
        launch: (2 K + 4) F T 4 bytes per chunk, about 1.1 GB for a 10 min recording at K = 5 (chunk_waveforms); there is no
        budget logic.  At another sample_rate the sample rows go up through the resampler in one batch with the other rows;
        the statistics are not formed there (a standard deviation does not pass through a resampler): ValueError.
        A chain of per-chunk Gaussians is not the recording's posterior; 'continuity' says where it means least."""
        if wave.dim() != 1:
            raise ValueError(f"wave {tuple(wave.shape)}: want one channel, [L]")
        c = self.config
        if c.match not in MATCH:
            raise ValueError(f"match = {c.match!r}: 'greedy' or 'sign'")
        sampling = int(samples) > 0 or coeffs is not None
        if not sampling and int(samples) < 0:
            raise ValueError(f"samples = {samples}: a count")
        if sampling:
            from .posterior import DOMAINS, MAX_STAT_S
            if domain not in DOMAINS:
                raise ValueError(f"domain must be one of {sorted(DOMAINS)}, got {domain!r}")
            if not (keep_samples or stats):
                raise ValueError("recording posterior: nothing asked for (keep_samples and stats are both off)")
            if coeffs is not None and (not isinstance(coeffs, torch.Tensor) or coeffs.dim() < 2):
                raise ValueError("coeffs is a tensor [S,K] (real or complex) or [S,K,2]")
            S = int(samples) if coeffs is None else int(coeffs.shape[0])
            if stats and not 2 <= S <= MAX_STAT_S:
                raise ValueError(f"statistics need 2 <= S <= {MAX_STAT_S} samples, got {S}")
        if sample_rate is not None and int(sample_rate) != int(c.sample_rate):
            if sampling and stats:
                raise ValueError("the sample statistics are formed at the model's rate only: a standard deviation does not "
                                 "pass through the resampler")
            more = dict(samples=samples, seed=seed, coeffs=coeffs, domain=domain, temperature=temperature) if sampling else {}
            return self._enhance_at_rate(wave, alphas, int(sample_rate), **more)
        plan = self.plan(wave.numel())
        H.require_gpu()
        x = wave.to(self.device).float().contiguous()
        if not sampling:
            buf = self.chunk_waveforms(x, plan, with_directions=alphas is not None)
            out = splice_chunks(buf[:, 0], buf[:, 1:], plan[-1][1], alphas, c.match)
        else:
            out = self._enhance_and_sample(x, plan, alphas, S, seed, coeffs, domain, temperature, keep_samples, stats)
        out["chunks"] = plan
        if alphas is not None:
            out["alphas"] = alphas if isinstance(alphas, torch.Tensor) else [float(a) for a in alphas]
        return out

    def _enhance_and_sample(self, x, plan, alphas, S, seed, coeffs, domain, temperature, keep_samples, stats):
        from .posterior import as_coefficients, draw_coefficients
        c, st = self.config, self._stft()
        n, last = len(plan), plan[-1][1]
        buf, planes = self.chunk_waveforms(x, plan, keep_planes=True)
        K = buf.shape[1] - 1
        if K < 1:
            raise ValueError("the model has no directions to sample along")
        if coeffs is not None:
            z = as_coefficients(coeffs[None])[0].to(self.device)
        else:
            z = draw_coefficients(1, S, K, seed=seed, temperature=temperature, device=self.device)[0]
        if alphas is not None:
            out = splice_chunks(buf[:, 0], buf[:, 1:], last, alphas, c.match)
        else:                                                                   # the tables as splice_chunks forms them
            out = {"enhanced": splice(buf[:, 0], None, last, None, None, None)[0]}
            work = boundary_gram(buf[:, 1:])[0] if n > 1 else None
            out["perm"], out["sign"], out["continuity"] = chain(work, n, K, c.match, device=buf.device)
        r = sample_chunks(planes["pred_crm"], planes["w_mat"], planes["re"], planes["im"], [ln for _, ln in plan], z, out["perm"],
                          out["sign"], last, c.chunk_samples, st.nfft, st.hop_length, domain=domain, samples=keep_samples,
                          stats=stats)
        out["coeffs"] = z
        if keep_samples:
            out["samples"] = r["samples"]
        if stats:
            out["sample_mean"], out["sample_std"] = r["mean"], r["std"]
        return out

    def _enhance_at_rate(self, wave, alphas, rate, **sampling):
        from . import resample as RSM
        c = self.config
        if rate <= 0:
            raise ValueError(f"sample_rate = {rate}: not a rate")
        for pair in ((rate, c.sample_rate), (c.sample_rate, rate)):
            t = RSM.sinc_table(*pair)
            if t.tile == 0:                                                     # before anything is launched
                raise RSM._unsupported(t, *pair)
        H.require_gpu()
        N = wave.numel()
        x = wave.to(self.device).float().contiguous()
        low = RSM.resample(x, rate, c.sample_rate, backend="hip")
        out = self.enhance(low, alphas, **sampling)
        rows, V = [out["enhanced"][None]], 0
        if "variations" in out:
            K, A = out["variations"].shape[:2]
            V = K * A
            rows.append(out["variations"].reshape(V, -1))
        if "samples" in out:
            rows.append(out["samples"])
        rows = torch.cat(rows) if len(rows) > 1 else rows[0]
        up = RSM.resample(rows.contiguous(), c.sample_rate, rate, backend="hip")[:, :N]
        out["enhanced_model_rate"] = out["enhanced"]
        out["enhanced"] = up[0]
        if "variations" in out:
            out["variations"] = up[1:1 + V].unflatten(0, (K, A))
        if "samples" in out:
            out["samples"] = up[1 + V:]
        out["sample_rate"] = rate
        return out

    def enhance_file(self, path, out_path, alphas=None, keep_rate=True, out_format="auto", verify_flac_md5=True, samples=0,
                     seed=None, flac_predictor="fixed"):
        """wav or flac -> wav or flac, as RecordingRestorer.restore_file reads and writes them: decoded to mono
        (data._decode_wav, data._decode_flac for a name ending in .flac), enhanced, written as 16-bit PCM; out_format "wav",
        "flac" or "auto" (flac when out_path ends in .flac).  keep_rate=True: the file is decoded at ITS rate and
        enhance(..., sample_rate=rate) returns that rate and sample count, band-limited to config.sample_rate / 2;
        keep_rate=False: decoded to config.sample_rate and written at it.  samples, seed: enhance's (the samples are in the
        dict; save_posterior_samples writes them).  flac_predictor: the FLAC encoder's predictor, "fixed" or "lpc"
        (flac.encode_pcm).  -> enhance's dict"""
        from .data import _decode_flac, _decode_wav
        from .flac import write_waves
        if out_format not in ("wav", "flac", "auto"):
            raise ValueError(f"out_format = {out_format!r}: 'wav', 'flac' or 'auto'")
        if out_format == "auto":
            out_format = "flac" if str(out_path).lower().endswith(".flac") else "wav"
        is_flac = str(path).lower().endswith(".flac")
        rate = self.config.sample_rate
        if keep_rate:
            if is_flac:
                from .flac import probe
                rate = int(probe(path).sample_rate)
            else:
                from scipy.io import wavfile
                rate = int(wavfile.read(str(path), mmap=True)[0])
        wave = _decode_flac(path, rate, verify_md5=verify_flac_md5) if is_flac else _decode_wav(path, rate)
        if wave is None:
            raise ValueError(f"{path} holds no samples")
        wave = torch.as_tensor(wave)
        out = self.enhance(wave, alphas, sample_rate=rate, samples=samples, seed=seed)
        out.setdefault("sample_rate", rate)
        write_waves([out_path], out["enhanced"][None].contiguous(), rate, out_format, predictor=flac_predictor)
        return out

    def save_variations(self, result, folder, fmt="flac", alphas=None, flac_predictor="fixed"):
        """enhance's dict -> <folder>/enhanced.<ext> and, when it holds 'variations' [K, A, L],
        <folder>/pc_<k+1>/alpha_<a:.1f>.<ext> (the layout of inpainting.restore's save_variations): 16-bit mono at the rate
        of the dict, through flac.write_waves (fmt "flac": every waveform encoded in one device call; "wav": the same
        samples).  alphas: the sweep, when the dict does not carry it.  flac_predictor: the FLAC encoder's predictor, "fixed"
        or "lpc" (flac.encode_pcm).  -> the paths written"""
        from .flac import write_waves
        rate = int(result.get("sample_rate", self.config.sample_rate))
        paths, waves = [os.path.join(str(folder), f"enhanced.{fmt}")], [result["enhanced"].reshape(1, -1)]
        if "variations" in result:
            var = result["variations"]
            K, A, L = var.shape
            alphas = result.get("alphas") if alphas is None else alphas
            alphas = [float(a) for a in (alphas.tolist() if hasattr(alphas, "tolist") else alphas or [])]
            if len(alphas) != A:
                raise ValueError(f"{len(alphas)} alphas for {A} variations per direction")
            paths += [os.path.join(str(folder), f"pc_{k + 1}", f"alpha_{a:.1f}.{fmt}") for k in range(K) for a in alphas]
            waves.append(var.reshape(K * A, L))
        for p in paths:
            os.makedirs(os.path.dirname(p), exist_ok=True)
        stack = torch.cat([w.to(self.device).float() for w in waves]) if fmt == "flac" else torch.cat([w.float().cpu() for w in waves])
        write_waves(paths, stack, rate, fmt, predictor=flac_predictor)
        return paths

    def save_posterior_samples(self, result, folder, fmt="flac", flac_predictor="fixed"):
        """enhance's dict with 'samples' [S, L] -> <folder>/posterior/sample_<s>.<ext> (the layout of
        NPPCAudioValidator.save_posterior_samples), 16-bit mono at the rate of the dict, as they are (not normalised), in one
        flac.write_waves call (flac_predictor: its predictor, "fixed" or "lpc").  -> the paths written"""
        from .flac import write_waves
        if "samples" not in result:
            raise ValueError("the dict holds no 'samples': call enhance(..., samples=S) with keep_samples=True")
        rate = int(result.get("sample_rate", self.config.sample_rate))
        rows = result["samples"]
        paths = [os.path.join(str(folder), "posterior", f"sample_{s}.{fmt}") for s in range(rows.shape[0])]
        os.makedirs(os.path.dirname(paths[0]), exist_ok=True)
        write_waves(paths, (rows.to(self.device) if fmt == "flac" else rows.cpu()).float().contiguous(), rate, fmt,
                    predictor=flac_predictor)
        return paths
