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
           "boundary_gram", "chain", "splice", "chain_host", "splice_host", "MAX_K", "MAX_SPLIT", "MATCH"]

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

    def chunk_waveforms(self, x, plan, with_directions=True):
        """x [L] (device) and its plan -> buf [n, K + 1, C] (or [n, 1, C]): per chunk the enhanced waveform e_c, then the
        waveform p_{c,k} of ops.crm_directions_to_spectrograms' direction k.  Chunks run through NPPCModel's ragged path
        (lengths=) in batches of chunk_batch, so a chunk's output does not depend on its batch; each batch ends in ONE
        ragged ops.istft launch of its (K + 1) b spectra.  Samples past the last chunk's length are not written."""
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
        buf = None
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
        return buf

    def enhance(self, wave, alphas=None, sample_rate=None):
        """wave [L] float (host or device) -> dict: 'enhanced' [L]; 'chunks' (plan_chunks' list); with `alphas` [A] also
        'variations' [K, A, L] (enhanced + alpha PC_k, the K directions aligned from chunk to chunk), 'perm' [n, K] int32,
        'sign' [n, K] int32 and 'continuity' [n - 1, K] fp64, device tensors (module docstring).
        The inverse STFT is linear, so e + alpha p IS the variation: K + 1 transforms per chunk serve every alpha.
        No host read beyond what NPPCModel's forward does.
        sample_rate: None or config.sample_rate runs exactly the above.  Another rate: the recording is resampled to
        config.sample_rate (nppc_audio.resample), enhanced there, and every output row is resampled back and cut to L; the
        WHOLE output is then band-limited to config.sample_rate / 2 (unlike restoration, which keeps the input outside its
        gaps, every sample of an enhanced recording comes from the nets).  'chunks' is the plan at the model's rate."""
        if wave.dim() != 1:
            raise ValueError(f"wave {tuple(wave.shape)}: want one channel, [L]")
        c = self.config
        if c.match not in MATCH:
            raise ValueError(f"match = {c.match!r}: 'greedy' or 'sign'")
        if sample_rate is not None and int(sample_rate) != int(c.sample_rate):
            return self._enhance_at_rate(wave, alphas, int(sample_rate))
        plan = self.plan(wave.numel())
        H.require_gpu()
        x = wave.to(self.device).float().contiguous()
        buf = self.chunk_waveforms(x, plan, with_directions=alphas is not None)
        out = splice_chunks(buf[:, 0], buf[:, 1:], plan[-1][1], alphas, c.match)
        out["chunks"] = plan
        if alphas is not None:
            out["alphas"] = alphas if isinstance(alphas, torch.Tensor) else [float(a) for a in alphas]
        return out

    def _enhance_at_rate(self, wave, alphas, rate):
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
        out = self.enhance(low, alphas)
        rows = out["enhanced"][None]
        if "variations" in out:
            K, A = out["variations"].shape[:2]
            rows = torch.cat([rows, out["variations"].reshape(K * A, -1)])
        up = RSM.resample(rows.contiguous(), c.sample_rate, rate, backend="hip")[:, :N]
        out["enhanced_model_rate"] = out["enhanced"]
        out["enhanced"] = up[0]
        if "variations" in out:
            out["variations"] = up[1:].unflatten(0, (K, A))
        out["sample_rate"] = rate
        return out

    def enhance_file(self, path, out_path, alphas=None, keep_rate=True, out_format="auto", verify_flac_md5=True):
        """wav or flac -> wav or flac, as RecordingRestorer.restore_file reads and writes them: decoded to mono
        (data._decode_wav, data._decode_flac for a name ending in .flac), enhanced, written as 16-bit PCM; out_format "wav",
        "flac" or "auto" (flac when out_path ends in .flac).  keep_rate=True: the file is decoded at ITS rate and
        enhance(..., sample_rate=rate) returns that rate and sample count, band-limited to config.sample_rate / 2;
        keep_rate=False: decoded to config.sample_rate and written at it.  -> enhance's dict"""
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
        out = self.enhance(wave, alphas, sample_rate=rate)
        out.setdefault("sample_rate", rate)
        write_waves([out_path], out["enhanced"][None].contiguous(), rate, out_format)
        return out

    def save_variations(self, result, folder, fmt="flac", alphas=None):
        """enhance's dict -> <folder>/enhanced.<ext> and, when it holds 'variations' [K, A, L],
        <folder>/pc_<k+1>/alpha_<a:.1f>.<ext> (the layout of inpainting.restore's save_variations): 16-bit mono at the rate
        of the dict, through flac.write_waves (fmt "flac": every waveform encoded in one device call; "wav": the same
        samples).  alphas: the sweep, when the dict does not carry it.  -> the paths written"""
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
        write_waves(paths, stack, rate, fmt)
        return paths
