"""GPU: the PNG encoder kernels (csrc/spec_png.hip) give byte for byte what the serial host encoder gives (which
tests/test_png_cpu.py holds to the restatement), for the cases of tests/png_cases.py as one ragged batch, image by image and
run after run.  The encoder's tile is 4096 bytes of filtered stream: `big`, `const2_big` and `twos_big` are six tiles each,
and `twos_big` is a single run across all of them.  Every test runs under a time limit of its own: a hang ends the process
with a traceback."""
import faulthandler
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases
from nppc_audio import png

pytestmark = pytest.mark.gpu
LIMIT = 120
CASES = png_cases.cases()
PAL = png.palette("viridis")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def device(names):
    return png.encode_indexed([torch.from_numpy(CASES[n]).cuda() for n in names], PAL, backend="hip")


@pytest.fixture(scope="module")
def batch():
    """(names, the device's files of the whole ragged batch), encoded once and shared (read-only)"""
    names = list(CASES)
    return names, device(names)


def first_diff(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def test_ragged_batch_equals_the_host_encoder(batch):
    names, got = batch
    host = png.encode_indexed([torch.from_numpy(CASES[n]) for n in names], PAL, backend="host")
    for n, g, h in zip(names, got, host):
        assert g == h, f"{n}: device and host differ (first at byte {first_diff(g, h)} of {len(g)} / {len(h)})"
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(g))), CASES[n]), n


def test_each_image_alone_equals_its_bytes_in_the_batch(batch):
    names, got = batch
    for n, g in zip(names, got):
        assert device([n]) == [g], f"{n}: alone it gives other bytes than in the batch"


def test_two_runs_are_equal(batch):
    names, got = batch
    assert device(names) == got
    assert device(names[::-1]) == got[::-1]


def test_host_tensors_stacked_input_and_value_checks():
    stack = torch.from_numpy(np.stack([CASES["const2"], CASES["const0"]]))
    want = png.encode_indexed(list(stack), PAL, backend="host")
    assert png.encode_indexed(stack, PAL, backend="hip") == want               # [N, H, W], from the host
    assert png.encode_indexed(stack.cuda(), PAL) == want                        # auto takes the device
    with pytest.raises(ValueError):
        png.encode_indexed([torch.zeros(3, 0, dtype=torch.uint8).cuda()], PAL, backend="hip")
    with pytest.raises(ValueError):
        png.encode_indexed([torch.zeros(2, 16385, dtype=torch.uint8).cuda()], PAL, backend="hip")
