#!/usr/bin/env python3
"""Generate the ragged-inference fixture (tests/golden/ragged_enh.npz / .json) by RUNNING THE REFERENCE (CPU).

Same rules as make_goldens.py: imports the reference from make_goldens.REF (with make_goldens' placeholder modules) and
writes data only.

- Five synthetic noisy clips of different lengths at the fsr_tiny STFT (nfft 64, hop 32, look-ahead 2): 288 samples
  (T = 10 frames, the shortest clip the largest TSSE kernel of 10 takes), and T + look_ahead = 127, 128, 129 and 134 (the
  last one crosses into a second 128-row tile).  Stored as int16 PCM, concatenated.
- The reference's ModelValidator.enhance_audio of each clip ALONE (batch size 1, as the reference validates), on the
  restorer weights of the fsr_tiny configuration (oracle/weights.py, seed 21) in a temporary checkpoint.

Usage:  python tests/golden/make_goldens_ragged.py
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
LENGTHS = [3970, 288, 4040, 4001, 4200]        # T = 125, 10, 127, 126, 132 frames at hop 32


def q16(x):
    return np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)


def main():
    import utils as ref_utils
    from use_pre_trained_model.model_validator.model_validator import ModelValidator, ModelValidatorConfig
    from FullSubNet_plus.speech_enhance.fullsubnet_plus.model.fullsubnet_plus import FullSubNetPlusConfig

    cfgj = json.load(open(os.path.join(HERE, "fsr_tiny.json")))["config"]
    spec = W.restorer_spec(num_freqs=cfgj["F"], sb_neighbors=cfgj["sbn"], sb_hidden=cfgj["sbh"])
    wts = W.make_weights(spec, cfgj["seed"])
    mcfg = dict(num_freqs=cfgj["F"], sb_num_neighbors=cfgj["sbn"], sb_model_hidden_size=cfgj["sbh"])
    ck = os.path.join(tempfile.mkdtemp(), "restorer.tar")
    torch.save({"model": MG.to_t(wts)}, ck)
    stft_cfg = ref_utils.StftConfig(nfft=cfgj["nfft"], hop_length=cfgj["hop"], win_length=cfgj["nfft"])
    mv = ModelValidator(ModelValidatorConfig(model_path=ck, model_configuration=FullSubNetPlusConfig(**mcfg), device="cpu",
                                             audio_config=ref_utils.AudioConfig(sr=SR, stft_configuration=stft_cfg)))
    pcm, clean_pcm, enh = [], [], []
    for i, n in enumerate(LENGTHS):
        noisy, clean = W.synth_batch(1, n, first_clip=70 + i)
        p, cp = q16(noisy[0]), q16(clean[0])
        x = torch.from_numpy(p.astype(np.float32) / 32768.0)
        c = torch.from_numpy(cp.astype(np.float32) / 32768.0)
        e = mv.enhance_audio(x, c)
        pcm.append(p), clean_pcm.append(cp), enh.append(np.asarray(e, np.float32).reshape(-1))
        assert enh[-1].shape == (n,)
    out = {"lengths": np.array(LENGTHS, np.int64), "noisy_pcm": np.concatenate(pcm), "clean_pcm": np.concatenate(clean_pcm),
           "enhanced": np.concatenate(enh)}
    np.savez_compressed(os.path.join(HERE, "ragged_enh.npz"), **out)
    meta = {"model_config": mcfg, "weights": "oracle/weights.py restorer_spec, seed of fsr_tiny.json",
            "stft": {"nfft": cfgj["nfft"], "hop": cfgj["hop"]}, "pcm_scale": 32768.0, "lengths": LENGTHS,
            "enhance": "reference ModelValidator.enhance_audio, one clip at a time"}
    json.dump(meta, open(os.path.join(HERE, "ragged_enh.json"), "w"), indent=1)
    print("written", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
