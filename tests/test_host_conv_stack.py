"""Host side of the fused encoder forward (csrc/pm_conv_stack.hip): which four-layer stacks the planner accepts, the LDS it
plans for them, and the argument checks in front of the launch.  No device is needed: nothing here launches."""
import ctypes as C

import pytest

from posterior_matching_amd import _lib, ops
from posterior_matching_amd.ops import ACT_LEAKY, ACT_RELU, LayerGeom

ALIGNED = 1 << 20            # never dereferenced: the checks only look at the values


def mnist_stack(c0, layers=((32, 5, 1), (32, 5, 2), (64, 5, 1), (64, 5, 2))):
    h, w, c, geoms = 28, 28, c0, []
    for f, k, s in layers:
        g = LayerGeom.conv(h, w, c, f, k, s, "SAME")
        geoms.append(g)
        h, w, c = g.OH, g.OW, f
    return geoms


def plan(descs):
    n = C.c_longlong(-1)
    rc = _lib.load().pm_conv_stack_plan(descs, len(descs), C.byref(n))
    return n.value if rc == 0 else None


def launch(descs, in_=ALIGNED, w0=ALIGNED, ws=(None, ALIGNED, ALIGNED, ALIGNED), bias=(ALIGNED,) * 4, out=(ALIGNED,) * 4):
    arr = lambda xs: (C.c_void_p * 4)(*xs)                                  # noqa: E731
    return _lib.load().pm_conv_stack_fwd_bf16(None, descs, len(descs), in_, w0, arr(ws), arr(bias), arr(out))


@pytest.mark.parametrize("c0", [1, 2])
def test_mnist_encoder_stacks_are_accepted(c0):
    geoms = mnist_stack(c0)
    for B in (1, 3, 128, 256):
        lds = plan(ops._conv_stack_descs(geoms, B))
        # region X: 28 x 28 x (32 + 8) hi / lo planes + zero slots (later the 14 x 14 x 72 planes of L3's output);
        # region Y: 14 x 14 x (32 + 8) planes of L2's output (first the f32 input patch, C0 x 32 x 32 floats)
        assert lds == 2 * (784 * 40 + 64) * 2 + 2 * (196 * 40 + 64) * 2 == 157312
        assert ops.conv_stack_lds(geoms, B) == lds
    assert ops.conv_stack_applies(geoms, 256) and not ops.conv_stack_applies(geoms, 64)


def test_planner_rejects_other_stacks():
    base = mnist_stack(1)
    assert ops.conv_stack_lds(base[:3], 256) is None                         # exactly four layers
    for layers in [((32, 3, 1), (32, 5, 2), (64, 5, 1), (64, 5, 2)),        # L1 kernel size
                   ((32, 5, 2), (32, 5, 1), (64, 5, 1), (64, 5, 2)),        # L1 stride
                   ((16, 5, 1), (32, 5, 2), (64, 5, 1), (64, 5, 2)),        # L1 width (lane = channel, 32)
                   ((32, 5, 1), (32, 5, 1), (64, 5, 1), (64, 5, 2)),        # another deal of tiles (L2 stride 1)
                   ((32, 5, 1), (32, 5, 2), (64, 5, 1), (64, 5, 1)),        # L4 stride
                   ((32, 5, 1), (48, 5, 2), (64, 5, 1), (64, 5, 2)),        # L3's input channels % 32
                   ((32, 5, 1), (32, 5, 2), (64, 5, 1), (66, 5, 2))]:       # N % 4 (TR epilogue)
        assert ops.conv_stack_lds(mnist_stack(1, layers), 256) is None, layers
    assert ops.conv_stack_lds(mnist_stack(3), 256) is None                   # C0 in {1, 2}
    # 28 x 28 x 64 planes after L1 would need 2 x 784 x 72 x 2 B = 226 KB of LDS
    d = ops._conv_stack_descs(base, 256)
    d[0].N, d[1].C = 64, 64
    assert plan(d) is None
    for field, value in [("out_act", ACT_RELU), ("in_act", ACT_LEAKY), ("B", 0), ("groups", 2), ("d", 2), ("cs", -1)]:
        for i in range(4):
            d = ops._conv_stack_descs(base, 256)
            setattr(d[i], field, value)
            assert plan(d) is None, (field, i)
    d = ops._conv_stack_descs(base, 256)
    for x in d:
        x.B = 0
    assert plan(d) is None                                                   # B >= 1
    d = ops._conv_stack_descs(base, 256)
    d[2].IH = 13                                                             # not a chain
    assert plan(d) is None
    assert _lib.load().pm_conv_stack_plan(None, 4, None) != 0


def test_launch_argument_checks_return_before_any_launch():
    d = ops._conv_stack_descs(mnist_stack(2), 256)
    assert launch(d, in_=None) != 0
    assert launch(d, w0=None) != 0
    assert launch(d, ws=(None, ALIGNED, None, ALIGNED)) != 0
    assert launch(d, ws=(None, ALIGNED, ALIGNED + 8, ALIGNED)) != 0          # 16-byte aligned weights
    assert launch(d, out=(ALIGNED, ALIGNED, ALIGNED + 4, ALIGNED)) != 0      # 16-byte aligned outputs
    assert launch(d, out=(ALIGNED, None, ALIGNED, ALIGNED)) != 0
    assert launch(d, bias=(ALIGNED, ALIGNED, ALIGNED, ALIGNED + 4)) != 0     # 16-byte aligned biases
    d[3].out_act = ACT_RELU                                                  # not the leaky stack
    assert launch(d) != 0
    d = ops._conv_stack_descs(mnist_stack(2), 256)
    assert _lib.load().pm_conv_stack_fwd_bf16(None, d, 3, ALIGNED, ALIGNED, None, None, None) != 0
