"""GPU: whole-recording enhancement: nppc_enh_gram, nppc_enh_chain and nppc_enh_splice against the
numpy restatement (tests/enhance_ref.py) on constructed directions, the invariance the alignment exists for, and
RecordingEnhancer.enhance against the same launch sequence composed by hand on the small model of the validation tests."""
import os

import numpy as np
import pytest
import torch

import enhance_ref as R
from golden_util import load
from nppc_validation_ref import clips, model_config

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
ULP64 = 2.0 ** -52
# `variations` (alpha applied AFTER the inverse STFT: e + alpha p) against ops.pc_direction_waveforms (alpha applied BEFORE
# it), relative to the peak of the variations.  Both are fp32 evaluations of one fp64 value; the test measures each against
# the fp64 evaluation of both orders on the same spectra (torch.istft on the CPU) and the two against each other.  Measured
# on the MI355X: see ORDER_MEASURED; the limit is 4 x the worst of the three.
ORDER_MEASURED = 1.56e-7          # after_vs_before; after_vs_fp64 1.06e-7, before_vs_fp64 1.18e-7; the fp64 orders 2.9e-16 apart
ORDER_LIMIT = 4 * ORDER_MEASURED


def E():
    from nppc_audio import enhance
    return enhance


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                    # a copy: the shared cases stay read-only


_cases = {}


def case(K, C, n):
    """one construction and one restatement per case, shared and left unchanged"""
    key = (K, C, n)
    if key not in _cases:
        enh, pcs, tp, ts = R.directions(K, C, n, R.SEEDS[key])
        perm, sign, cont, gap = R.chain(pcs)
        assert gap >= 0.1, (key, gap)                               # before anything is compared: no near-tie in these inputs
        assert np.array_equal(perm, tp) and np.array_equal(sign, ts)
        for a in (enh, pcs, perm, sign, cont):
            a.setflags(write=False)
        _cases[key] = dict(enh=enh, pcs=pcs, perm=perm, sign=sign, cont=cont)
    return _cases[key]


def gram_reference(pcs):
    n, K, C = pcs.shape
    G, na, nb, absG = R.gram(pcs)
    ref = np.concatenate([G.reshape(n - 1, -1), na, nb], axis=1)
    lim = 2 * (C // 2) * U53 * np.concatenate([absG.reshape(n - 1, -1), na, nb], axis=1)
    return ref, lim


def check_gram_and_chain(pcs, split, match="greedy"):
    en = E()
    n, K, C = pcs.shape
    work, S = en.boundary_gram(dev(pcs), split)
    assert S == en.enh_shape(n, K, C, split)[0] and tuple(work.shape) == (n - 1, S, K * (K + 2))
    perm, sign, cont, gram = en.chain(work, n, K, match, want_gram=True)
    ref, lim = gram_reference(pcs)
    err = np.abs(gram.cpu().numpy() - ref)
    assert np.all(err <= lim), (float((err - lim).max()), S)
    rp, rs, rc, _ = R.chain(pcs, match)
    assert np.array_equal(perm.cpu().numpy(), rp) and np.array_equal(sign.cpu().numpy(), rs)
    # |cos| = |G| / sqrt(na nb): the Gram bound carried through the quotient, to first order, plus 4 ulps of 1
    G, na, nb = ref[:, :K * K].reshape(n - 1, K, K), ref[:, K * K:K * K + K], ref[:, K * K + K:]
    bG, bna, bnb = lim[:, :K * K].reshape(n - 1, K, K), lim[:, K * K:K * K + K], lim[:, K * K + K:]
    got = cont.cpu().numpy()
    for c in range(1, n):
        for s in range(K):
            j, k = rp[c - 1, s], rp[c, s]
            d = na[c - 1, j] * nb[c - 1, k]
            if d == 0:
                assert got[c - 1, s] == 0
                continue
            bound = bG[c - 1, j, k] / np.sqrt(d) + rc[c - 1, s] * 0.5 * (bna[c - 1, j] / na[c - 1, j] + bnb[c - 1, k] / nb[c - 1, k])
            assert abs(got[c - 1, s] - rc[c - 1, s]) <= bound + 4 * ULP64, (c, s, got[c - 1, s], rc[c - 1, s], bound)
    return perm, sign, cont


# ---- Gram and chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,C,n", R.CASES)
@pytest.mark.parametrize("split", [0, 1, 64])
def test_gram_and_chain_on_the_constructed_cases(K, C, n, split):
    c = case(K, C, n)
    perm, sign, _ = check_gram_and_chain(c["pcs"], split)
    assert np.array_equal(perm.cpu().numpy(), c["perm"]) and np.array_equal(sign.cpu().numpy(), c["sign"])   # the truth
    check_gram_and_chain(c["pcs"], split, "sign")


@pytest.mark.parametrize("K,C,n,split", [(2, 2, 3, 0), (2, 2, 3, 64), (3, 514, 3, 0), (3, 514, 3, 1), (3, 514, 3, 64),
                                         (5, 2000, 4, 0), (5, 2000, 4, 1), (5, 2000, 4, 64), (16, 2000, 2, 3)])
def test_gram_at_sizes_that_are_no_multiple_of_a_tile(K, C, n, split):
    _, pcs, _, _ = R.directions(K, C, n, 5)
    work, S = E().boundary_gram(dev(pcs), split)
    gram = E().chain(work, n, K, want_gram=True)[3]
    ref, lim = gram_reference(pcs)
    err = np.abs(gram.cpu().numpy() - ref)
    assert np.all(err <= lim), (float((err - lim).max()), S)
    again = E().chain(E().boundary_gram(dev(pcs), split)[0], n, K, want_gram=True)[3]
    assert torch.equal(gram, again)                                 # a fixed order: the same bits twice


def test_chain_with_a_direction_that_is_zero_in_an_overlap():
    K, C, n = 3, 16, 3
    _, pcs, _, _ = R.directions(K, C, n, 11)
    pcs[1, 1, :C // 2] = 0
    pcs[1, 2, C // 2:] = 0
    perm, sign, cont = check_gram_and_chain(pcs, 0)
    perm, sign, cont = perm.cpu().numpy(), sign.cpu().numpy(), cont.cpu().numpy()
    s = int(np.flatnonzero(perm[1] == 2)[0])
    free = [k for k in range(K) if k not in perm[2][:s]]
    assert cont[1, s] == 0 and perm[2, s] == free[0] and sign[2, s] == sign[1, s]      # cosine 0, sign +1, lowest free index
    assert np.count_nonzero(cont[0] == 0) == 1


def test_one_chunk_has_the_identity():
    perm, sign, cont = E().chain(None, 1, 4, device="cuda")
    assert perm.tolist() == [[0, 1, 2, 3]] and sign.tolist() == [[1, 1, 1, 1]] and tuple(cont.shape) == (0, 4)


# ---- splice --------------------------------------------------------------------------------------------------------------
SPLICES = [  # K, C, n, last, alphas
    (2, 16, 1, 11, [1.0, -2.0]),          # one chunk, L < C
    (3, 16, 2, 9, [0.5, 1.5]),            # a last chunk of H + 1 samples
    (2, 16, 3, 16, [3.0, -0.25]),         # a full last chunk
    (3, 64, 4, 51, [1.0, 2.0]),           # L = 147, no multiple of 4
    (5, 18, 3, 13, [1.0, -1.0]),          # H = 9: a lane's four samples straddle the boundaries
    (2, 16, 3, 13, None),                 # A = 0: the enhanced row alone
    (8, 1024, 5, 1024, [0.7, -1.3]),      # several workgroups, 16-byte loads
    (16, 512, 3, 300, [2.0, 0.1]),
]


@pytest.mark.parametrize("K,C,n,last,alphas", SPLICES)
@pytest.mark.parametrize("match", ["greedy", "sign"])
@pytest.mark.parametrize("strided", [False, True])
def test_splice_is_the_restatement_bit_for_bit(K, C, n, last, alphas, match, strided):
    enh, pcs, _, _ = R.directions(K, C, n, 3)
    want, rp, rs, _ = R.enhance(enh, pcs, last, alphas, match)
    if strided:                                                     # views of one [n, K + 1, C + 3] buffer, as enhance passes them
        buf = torch.full((n, K + 1, C + 3), float("nan"), device="cuda")
        buf[:, 0, :C], buf[:, 1:, :C] = dev(enh), dev(pcs)
        e, p = buf[:, 0, :C], buf[:, 1:, :C]
    else:
        e, p = dev(enh), dev(pcs)
    out = E().splice_chunks(e, p, last, alphas, match)
    L = (n - 1) * (C // 2) + last
    assert tuple(out["enhanced"].shape) == (L,) and np.array_equal(bits(out["enhanced"]), bits(want[0]))
    if alphas is None:
        assert set(out) == {"enhanced"}
        return
    assert tuple(out["variations"].shape) == (K, len(alphas), L)
    assert np.array_equal(bits(out["variations"]).reshape(K * len(alphas), L), bits(want[1:]))
    assert out["perm"].dtype == torch.int32 and out["continuity"].dtype == torch.float64
    assert np.array_equal(out["perm"].cpu().numpy(), rp) and np.array_equal(out["sign"].cpu().numpy(), rs)
    assert tuple(out["continuity"].shape) == (n - 1, K)


def test_splice_into_rows_that_allow_no_vector_store():
    """the entry point on an output of odd row stride and an unaligned base: the scalar path gives the same bits"""
    from nppc_audio import _hip as H
    K, C, n, last = 3, 64, 4, 51
    enh, pcs, _, _ = R.directions(K, C, n, 3)
    alphas = np.array([1.0, 2.0], np.float32)
    want, rp, rs, _ = R.enhance(enh, pcs, last, alphas)
    L, V = (n - 1) * (C // 2) + last, 1 + K * 2
    store = torch.zeros(V * (L + 2) + 1, device="cuda")
    out = store[1:].view(V, L + 2)
    e, p = dev(enh), dev(pcs)
    H.call("nppc_enh_splice", e, C, p, K * C, C, n, K, C, L, dev(alphas), 2, E().hann_table(C, "cuda"), dev(rp), dev(rs),
           H.c_p(out.data_ptr()), L + 2, H.stream())
    assert np.array_equal(bits(out[:, :L]), bits(want)) and bool((out[:, L:] == 0).all())


# ---- the invariance the alignment exists for -----------------------------------------------------------------------------
@pytest.mark.parametrize("K,C,n", R.CASES[1:])
def test_signed_permutations_of_the_directions_change_nothing_but_only_with_alignment(K, C, n):
    en = E()
    c = case(K, C, n)
    alphas, last = [-2.0, 0.5, 3.0], C - 3
    perms, signs = R.signed_permutations(np.random.default_rng(1), n, K)
    moved = R.apply_signed(c["pcs"], perms, signs)
    base = en.splice_chunks(dev(c["enh"]), dev(c["pcs"]), last, alphas)
    again = en.splice_chunks(dev(c["enh"]), dev(moved), last, alphas)
    assert np.array_equal(bits(base["variations"]), bits(again["variations"]))
    assert np.array_equal(bits(base["enhanced"]), bits(again["enhanced"]))
    assert np.array_equal(perms[np.arange(n)[:, None], again["perm"].cpu().numpy()], base["perm"].cpu().numpy())
    # the fault itself: the same two inputs spliced with perm = identity and sign = +1 differ
    ident = torch.arange(K, dtype=torch.int32, device="cuda").repeat(n, 1)
    ones = torch.ones(n, K, dtype=torch.int32, device="cuda")
    plain = [en.splice(dev(c["enh"]), dev(p), last, alphas, ident, ones) for p in (c["pcs"], moved)]
    assert np.array_equal(bits(plain[0][0]), bits(plain[1][0]))                          # the enhanced row has no directions
    assert not np.array_equal(bits(plain[0][1:]), bits(plain[1][1:]))


# ---- end to end ----------------------------------------------------------------------------------------------------------
CHUNK = 1024                               # H = 512 >= hop x the largest TSSE kernel (32 x 10)


@pytest.fixture(scope="module")
def enhancer(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("enhance")
    c = load("g0_tiny")[1]["config"]
    cfg, wts = model_config(c, "fp32", tmp)
    ck = str(tmp / "nppc.pt")
    torch.save({"model_state_dict": wts, "step": 0}, ck)
    en = E()
    return en.RecordingEnhancer(en.RecordingEnhancerConfig(model_configuration=cfg, checkpoint_path=ck, chunk_samples=CHUNK,
                                                           chunk_batch=2)), c


def by_hand(enh, x, alphas):
    """enhance()'s launch sequence from the public pieces: ops.stft, NPPCModel, ops.istft, splice_chunks"""
    from nppc_audio import ops
    en, model, c = E(), enh.model, enh.config
    st = c.model_configuration.stft_configuration
    plan = R.plan(x.numel(), CHUNK)
    n, W = len(plan), (x.numel() if len(plan) == 1 else CHUNK)
    chunks = torch.zeros(n, W, device="cuda")
    for i, (s, ln) in enumerate(plan):
        chunks[i, :ln] = x[s:s + ln]
    K = None
    buf = None
    with torch.no_grad():
        for b0 in range(0, n, c.chunk_batch):
            xb = chunks[b0:b0 + c.chunk_batch]
            lens = [ln for _, ln in plan[b0:b0 + c.chunk_batch]]
            w_mat = model(xb, lengths=lens)
            crm = model.get_pred_crm(xb, lengths=lens)
            _, re, im = ops.stft(xb, st.nfft, st.hop_length, want_mag=False, lengths=lens)
            _, e_re, e_im = ops.cirm_decompress_apply(crm, re, im)
            d_re, d_im = ops.crm_directions_to_spectrograms(w_mat, re, im)
            K = d_re.shape[1]
            s_re, s_im = torch.cat((e_re[:, None], d_re), 1), torch.cat((e_im[:, None], d_im), 1)
            waves = ops.istft(s_re.flatten(0, 1), s_im.flatten(0, 1), st.nfft, st.hop_length, W,
                              lengths=[ln for ln in lens for _ in range(K + 1)])
            if buf is None:
                buf = torch.zeros(n, K + 1, CHUNK, device="cuda")
            buf[b0:b0 + len(lens), :, :W] = waves.view(len(lens), K + 1, W)
    return en.splice_chunks(buf[:, 0], buf[:, 1:], plan[-1][1], alphas, c.match), plan


def test_enhance_is_the_hand_composed_sequence(enhancer):
    enh, c = enhancer
    x = clips([2603])[0][0].cuda()                                  # 5 chunks in 3 batches, a last chunk of 555 samples
    alphas = [-3.0, 1.0, 2.5]
    out = enh.enhance(x, alphas)
    want, plan = by_hand(enh, x, alphas)
    assert out["chunks"] == plan and len(plan) == 5 and plan[-1] == (2048, 555)
    assert tuple(out["enhanced"].shape) == (2603,) and tuple(out["variations"].shape) == (c["K"], 3, 2603)
    for key in ("enhanced", "variations"):
        assert np.array_equal(bits(out[key]), bits(want[key])), key
    for key in ("perm", "sign", "continuity"):
        assert torch.equal(out[key], want[key]), key
    assert tuple(out["perm"].shape) == (5, c["K"]) and tuple(out["continuity"].shape) == (4, c["K"])
    assert bool(torch.isfinite(out["variations"]).all()) and float(out["continuity"].max()) <= 1 + 1e-12
    plain = enh.enhance(x.cpu())                                    # a host recording, no alphas: the enhanced row alone
    assert set(plain) == {"enhanced", "chunks"} and np.array_equal(bits(plain["enhanced"]), bits(out["enhanced"]))


def test_a_short_recording_is_the_ragged_clip(enhancer, record_err):
    from nppc_audio import ops
    enh, c = enhancer
    model, st = enh.model, enh.config.model_configuration.stft_configuration
    L = 1001
    x = clips([L], first=180)[0][0].cuda()
    alphas = [-3.0, -1.0, 0.5, 3.0]
    out = enh.enhance(x, alphas)
    assert out["chunks"] == [(0, L)] and out["perm"].tolist() == [list(range(c["K"]))] and out["sign"].tolist() == [[1] * c["K"]]
    with torch.no_grad():
        w_mat = model(x[None], lengths=[L])
        crm = model.get_pred_crm(x[None], lengths=[L])
        _, re, im = ops.stft(x[None], st.nfft, st.hop_length, want_mag=False, lengths=[L])
        clip = ops.model_outputs_to_waveforms(crm, re[:, None], im[:, None], L, st.nfft, st.hop_length, lengths=[L])
        T = 1 + L // st.hop_length
        _, before = ops.pc_direction_waveforms(crm[..., :T], w_mat[..., :T], alphas, re[..., :T], im[..., :T], L, st.nfft,
                                               st.hop_length)
        _, e_re, e_im = ops.cirm_decompress_apply(crm, re, im)
        d_re, d_im = ops.crm_directions_to_spectrograms(w_mat, re, im)
    assert np.array_equal(bits(out["enhanced"]), bits(clip[0]))
    # the two orders in fp64 on the same spectra
    win = torch.hann_window(st.nfft, periodic=True, dtype=torch.float64)
    inv = lambda z: torch.istft(z, st.nfft, st.hop_length, st.nfft, win, center=True, length=L)      # noqa: E731
    Ez = torch.complex(e_re[0, :, :T].double().cpu(), e_im[0, :, :T].double().cpu())
    Dz = torch.complex(d_re[0, :, :, :T].double().cpu(), d_im[0, :, :, :T].double().cpu())
    a64 = torch.tensor(alphas, dtype=torch.float64)
    first = inv((Ez[None, None] + a64[None, :, None, None] * Dz[:, None]).flatten(0, 1)).view(c["K"], len(alphas), L)
    after = inv(Ez[None])[0][None, None] + a64[None, :, None] * inv(Dz)[:, None]
    peak = float(first.abs().max())
    figures = {"fp64_orders": float((first - after).abs().max()) / peak,
               "after_vs_fp64": float((out["variations"].double().cpu() - first).abs().max()) / peak,
               "before_vs_fp64": float((before[0].double().cpu() - first).abs().max()) / peak,
               "after_vs_before": float((out["variations"] - before[0]).abs().max()) / peak}
    print("enhance order figures:", figures)
    assert figures["fp64_orders"] < 1e-13
    for tag in ("after_vs_fp64", "before_vs_fp64", "after_vs_before"):
        record_err(tag, figures[tag], ORDER_LIMIT)


def test_enhance_at_another_rate_is_down_enhance_up(enhancer):
    from nppc_audio import resample as RSM
    enh, c = enhancer
    N = 7001
    x = clips([N], first=185)[0][0].cuda()
    alphas = [-1.0, 2.0]
    out = enh.enhance(x, alphas, sample_rate=44100)
    low = RSM.resample(x, 44100, 16000, backend="hip")
    inner = enh.enhance(low, alphas)
    rows = torch.cat([inner["enhanced"][None], inner["variations"].reshape(-1, low.numel())]).contiguous()
    up = RSM.resample(rows, 16000, 44100, backend="hip")[:, :N]
    assert tuple(out["enhanced"].shape) == (N,) and tuple(out["variations"].shape) == (c["K"], 2, N)
    assert out["sample_rate"] == 44100 and out["chunks"] == inner["chunks"] and len(inner["chunks"]) > 1
    assert np.array_equal(bits(out["enhanced"]), bits(up[0]))
    assert np.array_equal(bits(out["variations"]).reshape(-1, N), bits(up[1:]))


def test_files_in_and_out(enhancer, tmp_path):
    """enhance_file and save_variations: wav in, flac out at the file's rate, the folder layout"""
    from scipy.io import wavfile
    from nppc_audio.flac import decode_files
    enh, c = enhancer
    x = clips([2603])[0][0]
    pcm = np.clip(np.rint(x.numpy() / np.abs(x.numpy()).max() * 0.5 * 32768.0), -32768, 32767).astype(np.int16)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.flac")
    wavfile.write(src, 16000, pcm)
    alphas = [-1.0, 1.0]
    out = enh.enhance_file(src, dst, alphas)
    direct = enh.enhance(torch.from_numpy(pcm.astype(np.float32) / 32768.0), alphas)
    assert np.array_equal(bits(out["enhanced"]), bits(direct["enhanced"]))
    (a,), (info,) = decode_files([dst], out="mono")
    assert info.sample_rate == 16000 and a.numel() == 2603
    want = np.clip(np.rint(out["enhanced"].cpu().double().numpy() * 32768.0), -32768, 32767) / 32768.0
    assert np.array_equal(a.numpy().astype(np.float64), want)
    paths = enh.save_variations(out, tmp_path / "v", fmt="flac")
    rel = sorted(str(p)[len(str(tmp_path / "v")) + 1:] for p in paths)
    assert rel == sorted(["enhanced.flac"] + [f"pc_{k + 1}/alpha_{a:.1f}.flac" for k in range(c["K"]) for a in alphas])
    assert all(os.path.getsize(p) > 0 for p in paths)
