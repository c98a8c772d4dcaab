#!/usr/bin/env python3
"""Generate the speech-enhancement metric fixtures (tests/golden/se_metrics.npz / .json) by RUNNING THE REFERENCE (CPU).

Same rules as make_goldens.py: runs only in the build container, imports the reference from /root/reference where it
lies (with make_goldens' placeholder modules, plus an empty `mir_eval.separation` that audio_zen/metrics.py imports and
never uses for SI_SDR), writes data only.

- Four clean / estimate pairs at 16 kHz (0.5 s, 1.3 s, 3 s, 4.7 s; int16 PCM, stored ragged) with silent stretches, a DC
  offset 100x the AC level, a scaled and low-passed estimate and an estimate equal to the reference.
- audio_zen.metrics.SI_SDR on float64 copies (so the recorded value carries no fp32 rounding): +inf for the equal pair.
- The SI-SDR of the reference's ModelValidator.calculate_metrics on float64 copies; the placeholders make pesq and stoi
  return 0 (pystoi is not available, so no STOI is recorded: the project states the STOI algorithm itself).
- ModelValidator.enhance_audio of two short synthetic clips, on the restorer weights of the fsr_tiny configuration
  (tests/golden/fsr_tiny.json: oracle/weights.py, seed 21), written to a temporary checkpoint the reference's
  utils.load_pretrained_model reads.

Usage:  python tests/golden/make_goldens_se_metrics.py
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402

MG.install_placeholders()
MG._placeholder("mir_eval")
MG._placeholder("mir_eval.separation", bss_eval_sources=lambda *a, **k: None)
sys.path.insert(0, MG.REF)
from oracle import weights as W  # noqa: E402

SR = 16000
LENGTHS = [8000, 20800, 48000, 75200]          # 0.5 s, 1.3 s, 3 s, 4.7 s


def speechlike(rng, n):
    """coloured noise under a 4 Hz envelope (the synth_clip recipe), peak ~0.3"""
    from scipy.signal import lfilter
    t = np.arange(n) / SR
    col = lfilter([0.05], [1.0, -0.95], rng.standard_normal(n))
    col /= np.std(col) + 1e-12
    env = 0.5 * (1.0 - np.cos(2 * np.pi * 4.0 * t + rng.uniform(0, 2 * np.pi)))
    return 0.05 * col * (0.2 + env)


def q16(x):
    return np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)


def make_pairs():
    from scipy.signal import lfilter
    rng = np.random.Generator(np.random.PCG64(2024))
    refs, ests = [], []
    # 0: 0.5 s, a silent stretch in the middle, estimate = clean + white noise at 5 dB SNR
    c = speechlike(rng, LENGTHS[0])
    c[3000:5000] = 0.0
    n = rng.standard_normal(LENGTHS[0])
    n *= np.sqrt(np.mean(c ** 2) / 10 ** 0.5 / np.mean(n ** 2))
    refs.append(c), ests.append(c + n)
    # 1: 1.3 s, two near-silent stretches, estimate = 0.3 x low-passed clean + a little noise
    c = speechlike(rng, LENGTHS[1])
    c[2000:6000] *= 1e-3
    c[14000:17000] = 0.0
    e = 0.3 * lfilter([0.5, 0.5], [1.0], c) + 0.002 * rng.standard_normal(LENGTHS[1])
    refs.append(c), ests.append(e)
    # 2: 3 s with a DC offset 100x the AC level on the reference, and a different offset on the estimate
    ac = 0.1 * speechlike(rng, LENGTHS[2])
    dc = 100.0 * np.sqrt(np.mean(ac ** 2))
    refs.append(ac + dc), ests.append(ac + 0.3 * ac[::-1] + 0.5 * dc)
    # 3: 4.7 s, a long silent stretch, estimate equal to the reference
    c = speechlike(rng, LENGTHS[3])
    c[30000:52000] = 0.0
    refs.append(c), ests.append(c.copy())
    return [q16(r) for r in refs], [q16(e) for e in ests]


def main():
    from FullSubNet_plus.speech_enhance.audio_zen import metrics as AZ
    import utils as ref_utils
    from use_pre_trained_model.model_validator.model_validator import ModelValidator, ModelValidatorConfig
    from FullSubNet_plus.speech_enhance.fullsubnet_plus.model.fullsubnet_plus import FullSubNetPlusConfig

    refs, ests = make_pairs()
    out = {"lengths": np.array(LENGTHS, np.int64),
           "ref_pcm": np.concatenate(refs), "est_pcm": np.concatenate(ests[:3])}   # pair 3: estimate = reference
    cfgj = json.load(open(os.path.join(HERE, "fsr_tiny.json")))["config"]
    spec = W.restorer_spec(num_freqs=cfgj["F"], sb_neighbors=cfgj["sbn"], sb_hidden=cfgj["sbh"])
    wts = W.make_weights(spec, cfgj["seed"])
    mcfg = dict(num_freqs=cfgj["F"], sb_num_neighbors=cfgj["sbn"], sb_model_hidden_size=cfgj["sbh"])
    ck = os.path.join(tempfile.mkdtemp(), "restorer.tar")
    torch.save({"model": MG.to_t(wts)}, ck)
    stft_cfg = ref_utils.StftConfig(nfft=cfgj["nfft"], hop_length=cfgj["hop"], win_length=cfgj["nfft"])
    mv = ModelValidator(ModelValidatorConfig(model_path=ck, model_configuration=FullSubNetPlusConfig(**mcfg), device="cpu",
                                             audio_config=ref_utils.AudioConfig(sr=SR, stft_configuration=stft_cfg)))
    sdr, sdr_zm = [], []
    with np.errstate(divide="ignore"):
        for r, e in zip(refs, ests):
            r64, e64 = r.astype(np.float32).astype(np.float64) / 32768.0, e.astype(np.float32).astype(np.float64) / 32768.0
            sdr.append(float(AZ.SI_SDR(r64, e64)))
            sdr_zm.append(float(mv.calculate_metrics(r64, e64)["SI_SDR"]))
    out["si_sdr"], out["si_sdr_zero_mean"] = np.array(sdr), np.array(sdr_zm)

    noisy, clean = W.synth_batch(2, 4096, first_clip=40)
    enh = [mv.enhance_audio(torch.from_numpy(noisy[i]), torch.from_numpy(clean[i])) for i in range(2)]
    out["enh_noisy"], out["enh_clean"], out["enhanced"] = noisy, clean, np.stack(enh).astype(np.float32)

    np.savez_compressed(os.path.join(HERE, "se_metrics.npz"), **out)
    meta = {"model_config": mcfg, "weights": "oracle/weights.py restorer_spec, seed of fsr_tiny.json",
            "stft": {"nfft": cfgj["nfft"], "hop": cfgj["hop"]}, "pcm_scale": 32768.0, "lengths": LENGTHS,
            "si_sdr": [repr(v) for v in sdr], "si_sdr_zero_mean": [repr(v) for v in sdr_zm]}
    json.dump(meta, open(os.path.join(HERE, "se_metrics.json"), "w"), indent=1)
    print("si_sdr", sdr, "\nsi_sdr_zero_mean", sdr_zm)


if __name__ == "__main__":
    main()
