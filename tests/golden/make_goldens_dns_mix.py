#!/usr/bin/env python3
"""Golden vectors for the DNS dynamic mixer by running the reference's own Dataset.snr_mix and Dataset.__getitem__
(fullsubnet_plus/dataset/dataset_train.py:130-207) on pre-loaded (name, waveform) lists: load_wav returns file[-1] for
such a pair, so nothing of the reference is replaced.  The object is built with Dataset.__new__ (the constructor only
reads path lists); `utils.logger`, which audio_zen/utils.py imports and the reference tree does not contain, gets an empty
stand-in like the other absent packages.  Python's `random` and numpy's legacy global stream are seeded per case.

Writes tests/golden/dns_mix.npz (clip pools and the reference's outputs) and dns_mix.json (per case: the decisions the
reference drew, CRC32 of the ingredients it mixed, and e_ref = max |reference fp32 - fp64 restatement| / peak, for the
convolution and for the final pair).  Asserted here: every case has | max|noisy| - 0.999 | > 1e-3 before the clip rule, so
a rounding difference can never flip the branch; seeds are searched until the reference itself satisfies it.
Runs only in the build container; data only."""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_goldens import REF, _placeholder, crc, install_placeholders  # noqa: E402
import dns_mix_ref as M  # noqa: E402

SR = 16000
SUB = 0.125                                        # seconds -> L = 2000
L = int(SUB * SR)
SILENCE = 0.01                                     # 160 samples
TARGET = -25
SNR_RANGE = (-5, 20)
CLEAN_LEN = [4500, 2000, 1200, 6000, 2001]         # longer than / equal to / shorter than the crop
NOISE_LEN = [700, 1300, 450]                       # several segments (+ silence) per item
MARGIN = 1e-3


def pools():
    rng = np.random.Generator(np.random.PCG64(2025))
    clean = [(0.1 * rng.standard_normal(n) * (0.3 + np.abs(np.sin(np.arange(n) / 500.0)))).astype(np.float32) for n in CLEAN_LEN]
    spiky = 0.01 * rng.standard_normal(L)          # a high crest factor: the mixture peaks above 0.999 at most levels
    spiky[[300, 900, 1500]] = [1.0, -0.8, 0.9]
    clean.append(spiky.astype(np.float32))
    noise = [(0.03 * (k + 1) * rng.standard_normal(n)).astype(np.float32) for k, n in enumerate(NOISE_LEN)]

    def decay(n, tau):
        return (rng.standard_normal(n) * np.exp(-np.arange(n) / tau)).astype(np.float32)
    rir = [decay(300, 60.0), np.stack([decay(800, 150.0) for _ in range(3)]), decay(2500, 600.0),
           np.array([0.7], dtype=np.float32)]
    return clean, noise, rir


def fit(a):
    a = a[:L]
    return np.append(a, np.zeros(L - len(a), dtype=np.float32)) if len(a) < L else a


def replay_draws(rir, floating):
    """the two draws snr_mix is about to make from numpy's global stream, read from a copy of its state"""
    rs = np.random.RandomState()
    rs.set_state(np.random.get_state())
    ch = int(rs.randint(0, rir.shape[0])) if (rir is not None and rir.ndim > 1) else -1
    return ch, int(rs.randint(TARGET - floating, TARGET + floating))


def measure(ref_noisy, ref_clean, clean, noise, snr, rir1d, level):
    """e_ref of the convolution and of the final pair, and the fp64 peak before the clip rule"""
    from scipy import signal
    e_conv = 0.0
    if rir1d is not None:
        e_conv = M.rel_peak(signal.fftconvolve(clean, rir1d)[:len(clean)], M.rir_convolve(clean, rir1d))
    info = {}
    n64, c64 = M.snr_mix(clean, noise, snr, TARGET, level, rir=rir1d, info=info)
    return dict(e_ref_conv=e_conv, e_ref_noisy=M.rel_peak(ref_noisy, n64), e_ref_clean=M.rel_peak(ref_clean, c64),
                peak_before_guard=info["peak_before_guard"], clipped=info["clipped"])


def main():
    install_placeholders()
    _placeholder("utils")
    _placeholder("utils.logger", log=print)
    sys.path.insert(0, REF)
    from FullSubNet_plus.speech_enhance.fullsubnet_plus.dataset.dataset_train import Dataset
    clean, noise, rir = pools()
    out = {f"clean{i}": c for i, c in enumerate(clean)}
    out.update({f"noise{i}": c for i, c in enumerate(noise)})
    out.update({f"rir{i}": c for i, c in enumerate(rir)})
    meta = dict(sr=SR, sub_sample_length=SUB, silence_length=SILENCE, target_dB_FS=TARGET, snr_range=list(SNR_RANGE),
                n_clean=len(clean), n_noise=len(noise), n_rir=len(rir), mix=[], items=[])

    # ---- Dataset.snr_mix directly: (name, clean, noise, rir, snr, floating, want the clip rule to fire)
    zeros = np.zeros(L, dtype=np.float32)
    mix_cases = [("dry", 0, 0, None, 5, 10, False), ("reverb", 0, 1, 0, 0, 10, False), ("rir2d", 3, 2, 1, 12, 3, False),
                 ("rir_longer", 1, 0, 2, -5, 10, False), ("rir_1tap", 4, 1, 3, 20, 3, False),
                 ("zero_noise", 0, None, 0, 7, 10, False), ("guard_dry", 5, 0, None, 15, 10, True),
                 ("guard_reverb", 5, 2, 0, 10, 10, True), ("spiky_low", 5, 1, None, 20, 3, None)]
    for name, ci, ni, ri, snr, floating, want_clip in mix_cases:
        c_in, n_in = fit(clean[ci]), (zeros if ni is None else fit(np.tile(noise[ni], 5)))
        r_in = None if ri is None else rir[ri]
        for seed in range(100, 200):
            np.random.seed(seed)
            ch, level = replay_draws(r_in, floating)
            ref_n, ref_c = Dataset.snr_mix(c_in.copy(), n_in.copy(), snr, TARGET, floating, rir=None if r_in is None else r_in.copy())
            r1 = None if r_in is None else (r_in[ch] if ch >= 0 else r_in)
            m = measure(ref_n, ref_c, c_in, n_in, snr, r1, level)
            if abs(m["peak_before_guard"] - 0.999) > MARGIN and want_clip in (None, m["clipped"]):
                break
        else:
            raise AssertionError(f"{name}: no seed keeps the clip rule {MARGIN} away from its threshold")
        assert ref_n.dtype == np.float32 or ref_n.dtype == np.float64
        out[f"mix.{name}.noisy"], out[f"mix.{name}.clean"] = ref_n.astype(np.float32), ref_c.astype(np.float32)
        meta["mix"].append(dict(name=name, clean=ci, noise=ni, rir=ri, snr=snr, floating=floating, seed=seed, channel=ch,
                                level=level, **m))

    # ---- Dataset.__getitem__: every clean clip, floating 3 and 10, RIRs for 3 of 4 items
    for floating in (3, 10):
        ds = Dataset.__new__(Dataset)
        ds.sr, ds.num_workers = SR, 0
        ds.clean_dataset_list = [(f"clean{i}", c) for i, c in enumerate(clean)]
        ds.noise_dataset_list = [(f"noise{i}", c) for i, c in enumerate(noise)]
        ds.rir_dataset_list = [(f"rir{i}", c) for i, c in enumerate(rir)]
        ds.snr_list = ds._parse_snr_range(SNR_RANGE)
        ds.reverb_proportion, ds.silence_length = 0.75, SILENCE
        ds.target_dB_FS, ds.target_dB_FS_floating_value, ds.sub_sample_length = TARGET, floating, SUB
        ds.length = len(clean)
        seen = {}
        real = Dataset.snr_mix

        def spy(clean_y, noise_y, snr, target_dB_FS, target_dB_FS_floating_value, rir=None, eps=1e-6):
            ch, level = replay_draws(rir, target_dB_FS_floating_value)
            seen.update(clean=clean_y.copy(), noise=noise_y.copy(), snr=int(snr), channel=ch, level=level,
                        rir=None if rir is None else (rir[ch] if ch >= 0 else rir).copy())
            return real(clean_y, noise_y, snr, target_dB_FS, target_dB_FS_floating_value, rir=rir, eps=eps)
        ds.snr_mix = spy
        for idx in range(len(clean)):
            for rep in range(2):
                start = 1000 * idx + 50 * rep + (500 if floating == 10 else 0)
                for seed in range(start, start + 50):
                    random.seed(seed)
                    np.random.seed(seed)
                    ref_n, ref_c = ds[idx]
                    m = measure(ref_n, ref_c, seen["clean"], seen["noise"], seen["snr"], seen["rir"], seen["level"])
                    if abs(m["peak_before_guard"] - 0.999) > MARGIN:
                        break
                else:
                    raise AssertionError(f"item {idx}: no seed keeps the clip rule away from its threshold")
                key = f"item.fl{floating}.i{idx}.s{seed}"
                out[key + ".noisy"], out[key + ".clean"] = ref_n, ref_c
                meta["items"].append(dict(key=key, idx=idx, floating=floating, seed=seed, snr=seen["snr"], level=seen["level"],
                                          channel=seen["channel"], rir_len=0 if seen["rir"] is None else len(seen["rir"]),
                                          crc_clean=crc(seen["clean"]), crc_noise=crc(seen["noise"]),
                                          crc_rir=0 if seen["rir"] is None else crc(seen["rir"]), **m))
    cases = meta["mix"] + meta["items"]
    assert all(abs(c["peak_before_guard"] - 0.999) > MARGIN for c in cases)
    assert any(c["clipped"] for c in cases) and any(not c["clipped"] for c in cases)
    assert any(c["rir_len"] == 0 for c in meta["items"]) and any(c["rir_len"] > 0 for c in meta["items"])
    np.savez_compressed(os.path.join(HERE, "dns_mix.npz"), **out)
    with open(os.path.join(HERE, "dns_mix.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(f"wrote {len(out)} arrays, {len(meta['mix'])} snr_mix cases, {len(meta['items'])} items; "
          f"clip rule fired in {sum(c['clipped'] for c in cases)}; worst e_ref conv "
          f"{max(c['e_ref_conv'] for c in cases):.2e}, noisy {max(c['e_ref_noisy'] for c in cases):.2e}, "
          f"clean {max(c['e_ref_clean'] for c in cases):.2e}; RIR lengths {sorted({c['rir_len'] for c in meta['items']})}")


if __name__ == "__main__":
    main()
