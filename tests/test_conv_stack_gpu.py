"""GPU: the one autograd chain of the 3x3 stack (ops._ConvBlock / ops._Conv / ops.frozen_block) in its two storage layouts,
fp32 NCHW (ops.NCHW) and bf16 P8 (p8.P8).

The block is VGG block 1 (3 -> 64 -> 64, pool) at the smallest map that still takes every route: n = 2, 8 x 16 pixels.  Layer 1
runs the direct stem kernel and the direct split-K weight gradient, layer 2 the F(4x4,3x3) kernel and the F(4x4,3x3)-domain weight
gradient (chunk fill 1.0 at 8 x 16); under operand rounding "bf16" both run the bf16-storage kernels.

LAUNCHES and SCANS below are literal: they were recorded with this file's own recorder (`_record`) on the commit BEFORE the two
chains were merged (ops._VGGBlock / ops._Conv3x3 and p8._Block / p8._Conv), so they pin the launch sequence, every non-pointer
argument, which pointers are null (the mask of epilogue 3 among them) and the anomaly reports of that commit."""
import contextlib
import ctypes

import pytest
import torch

from probabilisticteacher_amd import _lib, ops
from probabilisticteacher_amd.modeling.backbone import VGG, VGGBlock

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, H, W, CHANNELS = 2, 8, 16, (3, 64, 64)
MODES = {"fp32": None, "bf16": "bf16"}


class _Sink:
    """stands in for anomaly.AnomalySink: keeps what each scan was told"""

    def __init__(self):
        self.seen = []

    def scan(self, tensor, phase, op, output, branch="", scope="", p8=None):
        self.seen.append((phase, op, output, scope, p8))


@contextlib.contextmanager
def _spy(calls):
    """every _lib.call: (name, arguments) with a pointer as "p" and a null pointer as None"""
    call = _lib.call

    def spy(name, *a):
        calls.append((name, tuple(("p" if v.value else None) if isinstance(v, ctypes.c_void_p) else v for v in a)))
        return call(name, *a)
    _lib.call = spy
    try:
        yield calls
    finally:
        _lib.call = call


def _inputs():
    gen = torch.Generator().manual_seed(1711)
    x = torch.randn(N, CHANNELS[0], H, W, generator=gen)
    params = []
    for cin, cout in zip(CHANNELS, CHANNELS[1:]):
        params += [torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5, torch.randn(cout, generator=gen) * 0.1]
    gy = torch.randn(N, CHANNELS[-1], H // 2, W // 2, generator=gen)
    return x.to(DEV), [p.to(DEV) for p in params], gy.to(DEV)


def _train(run):
    """forward + backward of run(x, params) -> (y, dx, [dw1, db1, dw2, db2])"""
    x, params, gy = _inputs()
    x.requires_grad_()
    for p in params:
        p.requires_grad_()
    y = run(x, params)
    y.backward(gy)
    return y.detach(), x.grad, [p.grad for p in params]


def _block(x, params):
    return ops.vgg_block(x, True, params)


def _layers(x, params):
    for j in range(len(params) // 2):
        x = ops.conv3x3(x, params[2 * j], params[2 * j + 1], True)
    return ops.maxpool2x2(x)


def _frozen():
    """the block behind a frozen backbone: VGG.forward routes it to the path without a backward pass (epilogue 4)"""
    x, params, _ = _inputs()
    bb = VGG([VGGBlock(CHANNELS[0], CHANNELS[1:], pool=True)], out_features=["vgg_block1"]).to(DEV)
    with torch.no_grad():
        for p, v in zip(bb.vgg_block1[0].conv_params(), params):
            p.copy_(v)
    return bb.freeze(1)(x)["vgg_block1"]


def _record(mode):
    """everything the tests compare, for one operand-rounding mode, each run once"""
    out = {}
    with ops.operand_rounding(mode):
        with _spy([]) as calls:
            out["block"] = _train(_block)
        out["block_calls"] = calls
        with _spy([]) as calls:
            out["frozen"] = _frozen()
        out["frozen_calls"] = calls
        out["layers"] = _train(_layers)
        sink = _Sink()
        with ops.anomaly(sink), ops.anomaly_scope("blk"):
            _train(_block)
            _frozen()
        out["scans"] = sink.seen
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def recorded():
    """the launches below hold the kernel policy's defaults: set them for the recording, put back what was there"""
    before = ops._TILE_SCHEDULE, ops._WGRAD_WAVES, ops._P8_CONV_WAVES
    ops.set_tile_schedule("static"), ops.set_wgrad_waves(1), ops.set_p8_conv_waves(1)
    try:
        return {name: _record(mode) for name, mode in MODES.items()}
    finally:
        ops.set_tile_schedule(before[0]), ops.set_wgrad_waves(before[1]), ops.set_p8_conv_waves(before[2])


LAUNCHES = {('bf16', 'block'): [('ptmi_p8_from_nchw', ('p', 'p', 2, 3, 8, 16, None)),
                     ('ptmi_p8_pack_weights', ('p', 'p', 64, 3, 0, None)),
                     ('ptmi_p8_conv3x3_waves', ('p', 'p', 'p', None, 'p', 2, 3, 64, 8, 16, 1, 1, None)),
                     ('ptmi_p8_pack_weights', ('p', 'p', 64, 64, 0, None)),
                     ('ptmi_p8_conv3x3_waves', ('p', 'p', 'p', None, 'p', 2, 64, 64, 8, 16, 1, 1, None)),
                     ('ptmi_p8_maxpool2x2_fwd', ('p', 'p', 2, 64, 8, 16, None)),
                     ('ptmi_p8_to_nchw', ('p', 'p', 2, 64, 4, 8, None)),
                     ('ptmi_p8_from_nchw', ('p', 'p', 2, 64, 4, 8, None)),
                     ('ptmi_p8_maxpool2x2_bwd', ('p', 'p', 'p', 2, 64, 8, 16, 1, None)),
                     ('ptmi_p8_wgrad_waves', ('p', 'p', 'p', 'p', 'p', 2, 64, 64, 8, 16, 0, 1, None)),
                     ('ptmi_p8_pack_weights', ('p', 'p', 64, 64, 1, None)),
                     ('ptmi_p8_conv3x3_waves', ('p', 'p', None, 'p', 'p', 2, 64, 64, 8, 16, 3, 1, None)),
                     ('ptmi_p8_wgrad_waves', ('p', 'p', 'p', 'p', 'p', 2, 3, 64, 8, 16, 0, 1, None)),
                     ('ptmi_p8_pack_weights', ('p', 'p', 64, 3, 1, None)),
                     ('ptmi_p8_conv3x3_waves', ('p', 'p', None, None, 'p', 2, 64, 3, 8, 16, 2, 1, None)),
                     ('ptmi_p8_to_nchw', ('p', 'p', 2, 3, 8, 16, None))],
 ('bf16', 'frozen'): [('ptmi_p8_from_nchw', ('p', 'p', 2, 3, 8, 16, None)),
                      ('ptmi_p8_pack_weights', ('p', 'p', 64, 3, 0, None)),
                      ('ptmi_p8_conv3x3_waves', ('p', 'p', 'p', None, 'p', 2, 3, 64, 8, 16, 1, 1, None)),
                      ('ptmi_p8_pack_weights', ('p', 'p', 64, 64, 0, None)),
                      ('ptmi_p8_conv3x3_waves', ('p', 'p', 'p', None, 'p', 2, 64, 64, 8, 16, 4, 1, None)),
                      ('ptmi_p8_to_nchw', ('p', 'p', 2, 64, 4, 8, None))],
 ('fp32', 'block'): [('ptmi_conv3x3_pack_weights', ('p', 'p', 64, 3, 0, None)),
                     ('ptmi_conv3x3_fwd', ('p', 'p', 'p', None, 'p', 2, 3, 64, 8, 16, 1, None)),
                     ('ptmi_conv3x3_wino4p_pack_weights', ('p', 'p', 64, 64, 0, None)),
                     ('ptmi_conv3x3_wino4p_fwd_sched', ('p', 'p', 'p', None, 'p', 2, 64, 64, 8, 16, 1, None, None)),
                     ('ptmi_maxpool2x2_fwd', ('p', 'p', 128, 8, 16, None)),
                     ('ptmi_maxpool2x2_bwd', ('p', 'p', 'p', 128, 8, 16, 1, None)),
                     ('ptmi_conv3x3_wino4_wgrad_waves', ('p', 'p', 'p', 'p', 'p', 2, 64, 64, 8, 16, 0, 1, None)),
                     ('ptmi_conv3x3_wino4p_pack_weights', ('p', 'p', 64, 64, 1, None)),
                     ('ptmi_conv3x3_wino4p_fwd_sched', ('p', 'p', None, 'p', 'p', 2, 64, 64, 8, 16, 3, None, None)),
                     ('ptmi_conv3x3_wgrad', ('p', 'p', 'p', 'p', 'p', 2, 3, 64, 8, 16, 0, None)),
                     ('ptmi_conv3x3_wino4p_pack_weights', ('p', 'p', 64, 3, 1, None)),
                     ('ptmi_conv3x3_wino4p_fwd_sched', ('p', 'p', None, None, 'p', 2, 64, 3, 8, 16, 2, None, None))],
 ('fp32', 'frozen'): [('ptmi_conv3x3_pack_weights', ('p', 'p', 64, 3, 0, None)),
                      ('ptmi_conv3x3_fwd', ('p', 'p', 'p', None, 'p', 2, 3, 64, 8, 16, 1, None)),
                      ('ptmi_conv3x3_wino4p_pack_weights', ('p', 'p', 64, 64, 0, None)),
                      ('ptmi_conv3x3_wino4p_fwd_sched', ('p', 'p', 'p', None, 'p', 2, 64, 64, 8, 16, 4, None, None))]}
SCANS = {'bf16': [('forward', 'p8_from_nchw', 't', 'blk', (2, 3, 8, 16)),
          ('forward', 'p8_block', 'y', 'blk.conv1', (2, 64, 8, 16)),
          ('forward', 'p8_block', 'y', 'blk.conv2', (2, 64, 8, 16)),
          ('forward', 'p8_block', 'pooled', 'blk', (2, 64, 4, 8)),
          ('forward', 'p8_to_nchw', 'y', 'blk', None),
          ('backward', 'p8_to_nchw', 'dt', 'blk', (2, 64, 4, 8)),
          ('backward', 'p8_block', 'dz', 'blk.conv2', (2, 64, 8, 16)),
          ('backward', 'p8_block', 'dw', 'blk.conv2', None),
          ('backward', 'p8_block', 'db', 'blk.conv2', None),
          ('backward', 'p8_block', 'dz', 'blk.conv1', (2, 64, 8, 16)),
          ('backward', 'p8_block', 'dw', 'blk.conv1', None),
          ('backward', 'p8_block', 'db', 'blk.conv1', None),
          ('backward', 'p8_block', 'dx', 'blk.conv1', (2, 3, 8, 16)),
          ('backward', 'p8_from_nchw', 'dx', 'blk', None),
          ('forward', 'p8_to_nchw', 'y', 'blk.vgg_block1', None)],
 'fp32': [('forward', 'vgg_block', 'y', 'blk.conv1', None),
          ('forward', 'vgg_block', 'y', 'blk.conv2', None),
          ('forward', 'vgg_block', 'pooled', 'blk', None),
          ('backward', 'vgg_block', 'dz', 'blk.conv2', None),
          ('backward', 'vgg_block', 'dw', 'blk.conv2', None),
          ('backward', 'vgg_block', 'db', 'blk.conv2', None),
          ('backward', 'vgg_block', 'dz', 'blk.conv1', None),
          ('backward', 'vgg_block', 'dw', 'blk.conv1', None),
          ('backward', 'vgg_block', 'db', 'blk.conv1', None),
          ('backward', 'vgg_block', 'dx', 'blk.conv1', None),
          ('forward', 'conv3x3', 'y', 'blk.vgg_block1.0.conv1', None)]}


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("what", ["block", "frozen"])
def test_launch_sequence_is_the_recorded_one(recorded, name, what):
    """forward + backward of the block node, and the frozen block: every launch and its arguments, as recorded before the merge"""
    got, want = recorded[name][what + "_calls"], LAUNCHES[name, what]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"launch {i}: {a}, recorded {b}"
    assert len(got) == len(want), f"{len(got)} launches, recorded {len(want)}: {got[len(want):] or want[len(got):]}"


@pytest.mark.parametrize("name", list(MODES))
def test_anomaly_scans_are_the_recorded_ones(recorded, name):
    """(phase, op, output, scope, P8 shape) of every scan of one forward + backward of the block node, then of the frozen block"""
    assert recorded[name]["scans"] == SCANS[name]


@pytest.mark.parametrize("name", list(MODES))
def test_block_node_equals_the_block_layer_by_layer(recorded, name):
    """Bit for bit: one kernel set on one device.  The layer-by-layer chain (ops.conv3x3 x 2, ops.maxpool2x2) runs the plain pool
    backward, ptmi_relu_bwd and dgrad epilogue 2 where the block node runs the masked pool backward and dgrad epilogue 3: a mask
    selects, it does not round, so the gradients keep their bits as well."""
    (y, dx, grads), (yl, dxl, gradsl) = recorded[name]["block"], recorded[name]["layers"]
    assert not torch.isnan(y).any() and torch.equal(y, yl), "block output"
    for what, a, b in zip(("dw1", "db1", "dw2", "db2"), grads, gradsl):
        assert not torch.isnan(a).any() and torch.equal(a, b), what
    assert not torch.isnan(dx).any() and torch.equal(dx, dxl), "dx"
    assert torch.equal(recorded[name]["frozen"], y), "the frozen block (pool in the last epilogue) against the block node"
