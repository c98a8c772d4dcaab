"""CPU: host logic of ragged inference: pad_collate / RaggedBatch, frame-count arithmetic, argument
checks, and the new C-ABI entries."""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pad_collate_zero_pads_to_longest_and_keeps_lengths():
    from nppc_audio.data import RaggedBatch, pad_collate
    items = [(torch.ones(5), 2 * torch.ones(5)), (torch.arange(3.0), torch.arange(3.0)), (torch.ones(7), torch.ones(7), "x.wav")]
    b = pad_collate(items)
    assert isinstance(b, RaggedBatch) and isinstance(b, tuple)
    assert b.noisy.shape == (3, 7) and b.clean.shape == (3, 7)
    assert b.lengths.tolist() == [5, 3, 7] and b.lengths.dtype == torch.int64
    assert b.noisy[1].tolist() == [0, 1, 2, 0, 0, 0, 0]
    assert b.clean[0].tolist() == [2] * 5 + [0, 0]
    noisy, clean, lengths = b                     # unpacks like a tuple
    assert noisy is b.noisy and lengths is b.lengths
    with pytest.raises(ValueError, match="item 0"):
        pad_collate([(torch.ones(4), torch.ones(5))])
    with pytest.raises(ValueError):
        pad_collate([])


def test_ragged_batches_are_recognised_by_type_only():
    from nppc_audio.data import RaggedBatch, pad_collate
    plain = (torch.zeros(2, 8), torch.zeros(2, 8), torch.tensor([8, 8]))     # a reference item (noisy, clean, name, ...)
    assert not isinstance(plain, RaggedBatch)
    loader = torch.utils.data.DataLoader([(torch.ones(n), torch.ones(n)) for n in (4, 9, 6)], batch_size=2,
                                         collate_fn=pad_collate)
    batches = list(loader)
    assert all(isinstance(b, RaggedBatch) for b in batches)
    assert [b.lengths.tolist() for b in batches] == [[4, 9], [6]]


def test_frame_counts():
    from nppc_audio import ops
    assert ops.stft_frames(16000, 256) == 63
    assert ops.stft_frames([288, 3970, 4001, 4040], 32) == [10, 125, 126, 127]
    assert ops.stft_frames(torch.tensor([255, 256, 257]), 256).tolist() == [1, 2, 2]


def test_length_and_frame_checks():
    from nppc_audio import ops
    from nppc_audio.fullsubnet import check_frames
    dl, host = ops.ragged_lengths(torch.tensor([300, 40]), 2, 300, 32, "cpu")
    assert host == [300, 40] and dl.dtype == torch.int32 and dl.tolist() == [300, 40]
    with pytest.raises(ValueError, match="item 1"):
        ops.ragged_lengths([300, 32], 2, 300, 32, "cpu")                # L_b must exceed nfft // 2
    with pytest.raises(ValueError, match="item 0"):
        ops.ragged_lengths([301, 100], 2, 300, 32, "cpu")               # longer than the padded rows
    with pytest.raises(ValueError, match="entries"):
        ops.ragged_lengths([300], 2, 300, 32, "cpu")
    check_frames([10, 20], 2, 20, [3, 5, 10])
    with pytest.raises(ValueError, match="item 0"):
        check_frames([9, 20], 2, 20, [3, 5, 10])                        # fewer frames than the largest TSSE kernel
    with pytest.raises(ValueError, match="item 1"):
        check_frames([10, 21], 2, 20, [3, 5, 10])
    with pytest.raises(ValueError, match="entries"):
        check_frames([10], 2, 20, [3, 5, 10])


def test_ragged_entry_points_are_declared():
    from nppc_audio import _hip
    hdr = open(os.path.join(HERE, "..", "include", "nppc_hip.h")).read()
    for name in ("nppc_stft_ragged", "nppc_istft_ragged", "nppc_tsse_fwd_maps_ragged", "nppc_tcn_dwconv_ragged",
                 "nppc_tcn_gn_stats_ragged", "nppc_subband_mean_ragged", "nppc_crop_frames_ragged", "nppc_crm_mse_ragged"):
        assert f"int {name}(" in hdr and name in _hip.SIGS
