"""CPU: the launch trace of `UNetEngine` and of the clipped flat Adam step of the three trainers that use it, pinned against
tests/golden/unet_engine_calls.json.

The engine only orders launches and owns buffers, so it can be driven on CPU tensors with `H.call`, `H.require_gpu` and
`H.stream` replaced.  Every launch is kept as [name, args]; a tensor argument becomes ["T", i, storage offset, dtype, storage
bytes] with i the index of its storage in order of first appearance, so the trace also pins which launches share a buffer.
The whole trace must equal the golden one: names, order, scalars, offsets, dtypes and sizes.

The golden file is this recorder's own output.  To record it again (only with a change that is meant to alter the launches):
    PYTHONPATH=generative-audio_amd python tests/test_unet_engine_calls_cpu.py
"""
import contextlib
import json
import os
import types

import pytest
import torch
import torch.nn as nn

from nppc_audio import _hip as H
from nppc_audio import ops_lstm
from nppc_audio import restorer_trainer
from nppc_audio import trainer as T
from nppc_audio.engine import FlatParams
from nppc_audio.inpainting.networks.unet import UNet, UNetConfig
from nppc_audio.inpainting.trainer import nppc_trainer, restoration_trainer
from nppc_audio.unet_engine import UNetEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_engine_calls.json")
DROP = dict(p=0.2, seed=5, pass_id=7, tap=None)

# id: (in_ch, out_ch, precision, (B, F, T), dropout, xin given, expected ksplit)
ENGINE_CASES = {
    "restorer_1to1_bf16_drop_2x17x33": (1, 1, "bf16", (2, 17, 33), True, True, [1, 1, 1, 1, 1]),
    "directions_2to5_bf16_1x16x16": (2, 5, "bf16", (1, 16, 16), False, False, [1, 1, 1, 1, 1]),
    "directions_2to12_fp32_2x66x68": (2, 12, "fp32", (2, 66, 68), False, False, [8, 2, 1, 1, 1]),
    "directions_2to5_bf16_drop_2x30x40": (2, 5, "bf16", (2, 30, 40), True, False, [2, 1, 1, 1, 1]),
}
TRAINERS = ("InpaintingTrainer", "NPPCAudioInpaintingTrainer", "FullSubNetPlusTrainer")


class _Recorder:
    def __init__(self):
        self.calls = []
        self._index = {}
        self._alive = []        # a freed storage's address could be handed out again: keep every tensor seen

    def _arg(self, a):
        if isinstance(a, torch.Tensor):
            st = a.untyped_storage()
            i = self._index.setdefault(st._cdata, len(self._index))
            self._alive.append(a)
            return ["T", i, a.storage_offset(), str(a.dtype).replace("torch.", ""), st.nbytes()]
        if a is None or type(a) in (int, float, str):
            return a
        if hasattr(a, "_obj"):   # ctypes.byref(c_long): a *_elems query; answer it so that the scratch it sizes is not empty
            a._obj.value = 256
        return type(a).__name__

    def call(self, name, *args):
        self.calls.append([name, [self._arg(a) for a in args]])


@contextlib.contextmanager
def _recording():
    rec = _Recorder()
    saved = (H.call, H.require_gpu, H.stream, ops_lstm.check_coop_timeouts)
    H.call, H.require_gpu, H.stream = rec.call, lambda: None, lambda: "stream"
    ops_lstm.check_coop_timeouts = lambda what: rec.calls.append(["check_coop_timeouts", [what]])
    try:
        yield rec
    finally:
        H.call, H.require_gpu, H.stream, ops_lstm.check_coop_timeouts = saved


def _engine_trace(case):
    """eval forward, then two train steps (forward + backward): the second shows what is not packed again and that the
    gradient buffers alternate"""
    in_ch, out_ch, precision, (B, F, T), dropout, with_xin, ksplit = ENGINE_CASES[case]
    torch.manual_seed(0)
    net = UNet(UNetConfig(in_channels=in_ch, out_channels=out_ch, dropout=0.2 if dropout else 0.0, precision=precision))
    maps = [torch.zeros(B, F * T) for _ in range(in_ch)]
    mask, out, dout = torch.zeros(B, T), torch.zeros(B, out_ch, F, T), torch.zeros(B, out_ch, F, T)
    xin = dict(xin=maps[0], xin_bstride=F * T) if with_xin else {}
    with _recording() as rec:
        eng = UNetEngine(net, in_ch, out_ch, H.PREC_BF16 if precision == "bf16" else H.PREC_F32, True)
        eng.forward((B, F, T), maps, F * T, mask, out, F * T, **xin)
        for step in range(2):
            drop = dict(DROP, pass_id=DROP["pass_id"] + step) if dropout else None
            eng.forward((B, F, T), maps, F * T, mask, out, F * T, train=True, dropout=drop, **xin)
            eng.backward(dout, F * T)
    assert eng.ksplit == ksplit and eng.lv[0] == (F, T) and eng.dev == torch.device("cpu") and eng.fp.grad is not None
    return rec.calls


def _trainer_trace(which):
    """two train_steps of a trainer whose net is a 3 -> 2 linear layer and whose base_step is the sum of its parameters"""
    net = nn.Linear(3, 2)
    eng = types.SimpleNamespace(fp=FlatParams(net, "cpu"))
    eng.fp.grad = torch.zeros_like(eng.fp.flat)
    net.engine, net.flat_grad_only = (lambda: eng), False
    if which == "InpaintingTrainer":
        tr = restoration_trainer.InpaintingTrainer.__new__(restoration_trainer.InpaintingTrainer)
        nn.Module.__init__(tr)
        tr.model, tr.config = types.SimpleNamespace(net=net), types.SimpleNamespace(max_grad_norm=5.0)
        tr.base_step = lambda batch: (sum(p.sum() for p in net.parameters()), {})
    elif which == "NPPCAudioInpaintingTrainer":
        tr = nppc_trainer.NPPCAudioInpaintingTrainer.__new__(nppc_trainer.NPPCAudioInpaintingTrainer)
        nn.Module.__init__(tr)
        tr.nppc_model = types.SimpleNamespace(pc_wrapper=types.SimpleNamespace(net=net))
        tr.config = types.SimpleNamespace(max_grad_norm=1.0)
        tr.base_step = lambda batch: (torch.zeros(2), sum(p.sum() for p in net.parameters()), {})
    else:
        tr = restorer_trainer.FullSubNetPlusTrainer.__new__(restorer_trainer.FullSubNetPlusTrainer)
        nn.Module.__init__(tr)
        tr.model, tr.config = net, types.SimpleNamespace(clip_grad_norm_value=10)
        tr.base_step = lambda batch: (sum(p.sum() for p in net.parameters()), {})
    tr.optimizer, tr.step, tr._clip_step = T.HipAdam(net.parameters(), lr=1e-3, weight_decay=0.5), 0, T.ClippedFlatStep()
    logs = []
    with _recording() as rec:
        for _ in range(2):
            logs.append(tr.train_step(None)[-1])
    assert tr.step == 2 and not net.flat_grad_only
    return rec.calls, logs


def _all_traces():
    out = {"engine": {c: _engine_trace(c) for c in ENGINE_CASES}, "trainers": {w: _trainer_trace(w)[0] for w in TRAINERS}}
    return json.loads(json.dumps(out))        # tuples -> lists, as the golden file has them


def record_golden():
    traces = _all_traces()
    with open(GOLDEN, "w") as f:
        f.write("{\n")
        for gi, (group, cases) in enumerate(traces.items()):
            f.write(f' "{group}": {{\n')
            for ci, (case, calls) in enumerate(cases.items()):
                f.write(f'  "{case}": [\n')
                f.write(",\n".join("   " + json.dumps(c, separators=(",", ":")) for c in calls))
                f.write("\n  ]" + ("," if ci + 1 < len(cases) else "") + "\n")
            f.write(" }" + ("," if gi + 1 < len(traces) else "") + "\n")
        f.write("}\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _assert_same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what}: launch {k} differs\n got  {g}\n want {w}"
    assert len(got) == len(want), f"{what}: {len(got)} launches, the golden trace has {len(want)}"


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_launch_trace(golden, case):
    got = json.loads(json.dumps(_engine_trace(case)))
    assert len(got) >= 400
    _assert_same(got, golden["engine"][case], case)


@pytest.mark.parametrize("which", TRAINERS)
def test_trainer_clipped_step_calls(golden, which):
    calls, logs = _trainer_trace(which)
    got = json.loads(json.dumps(calls))
    tail = [["check_coop_timeouts", ["step 1"]], ["check_coop_timeouts", ["step 2"]]] if which == "FullSubNetPlusTrainer" else []
    # per step: the sum of squares of the flat gradient into one fp64 cell, then the clipped Adam that reads the cell
    assert [n for n, _ in got if n != "check_coop_timeouts"] == ["nppc_sumsq", "nppc_adam_step_clip"] * 2
    assert [c for c in got if c[0] == "check_coop_timeouts"] == tail
    max_norm = {"InpaintingTrainer": 5.0, "NPPCAudioInpaintingTrainer": 1.0, "FullSubNetPlusTrainer": 10.0}[which]
    steps = [c for c in got if c[0] != "check_coop_timeouts"]
    for t, (sumsq, adam) in enumerate(zip(steps[0::2], steps[1::2]), start=1):
        grad, cell = sumsq[1][0], sumsq[1][2]
        assert sumsq[1] == [grad, 8, cell, "stream"] and grad[3] == "float32" and cell[2:] == [0, "float64", 8]
        flat, m, v = adam[1][0], adam[1][2], adam[1][3]
        assert adam[1] == [flat, grad, m, v, 8, 1e-3, 0.9, 0.999, 1e-8, 0.5, t, 1.0, cell, max_norm, "stream"]
        assert len({flat[1], grad[1], m[1], v[1], cell[1]}) == 5
    assert steps[0][1] == steps[2][1] and steps[1][1][:10] == steps[3][1][:10]      # one cell, one stepper, over both steps
    for log in logs:
        assert ("grad_norm" in log) == (which != "NPPCAudioInpaintingTrainer")
        if "grad_norm" in log:
            assert log["grad_norm"].dtype == torch.float64 and log["grad_norm"].shape == (1,)
    _assert_same(got, golden["trainers"][which], which)


if __name__ == "__main__":
    record_golden()
