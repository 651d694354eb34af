"""What scan_mnist_kernel's dispatch needs no GPU for: the shape predicate of the dispatcher (through the library's host
export) and the iteration cost model of ips_amd/dist.py."""

import ctypes
import itertools

from ips_amd import dist, hip


def test_shape_predicate_is_true_at_the_mnist_shape_only():
    fn = hip.lib().ipsx_dbg_scan_mnist_shape
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    sizes, heads, tokens = (16, 63, 64, 65, 100, 128, 256), (1, 4, 8, 16, 32), (1, 2, 4, 8)
    for m, i, h, t in itertools.product(sizes, sizes, heads, tokens):
        assert fn(m, i, h, t) == (1 if (m, i, h, t) == (64, 64, 8, 4) else 0), (m, i, h, t)
    assert hip.scan_mnist_shape(64, 64, 8, 4)
    # 32 logits per candidate and 128 candidates in other arrangements are scan_fast_kernel's
    for shape in ((64, 64, 4, 8), (64, 64, 32, 1), (64, 64, 8, 1), (100, 28, 8, 4), (32, 96, 8, 4), (256, 256, 8, 1)):
        assert not hip.scan_mnist_shape(*shape), shape


def test_iteration_cost_model_has_the_mnist_entry():
    t = dist.loop_iteration_us(64, 64, 8, 4)
    assert t == dist.LOOP_US_MNIST
    assert 0.5 < t < 6.6                                              # below the general kernel's 2.5 + L R / 1000 at this shape
    assert dist.loop_iteration_us(256, 256, 8, 1) == 4.2              # scan_cam_kernel's entry stays
    assert abs(dist.loop_iteration_us(64, 80, 8, 4) - (2.5 + 144 * 32 / 1000.0)) < 1e-9      # other shapes: the general kernel
