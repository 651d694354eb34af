"""The patch-grid view on the GPU: the stems read their patches straight from the image grid.

Yardstick everywhere: the existing patch path on ``hip.patchify(images, ...)``, compared with ``torch.equal`` - behind the
staged image the view kernels run the code of the patch kernels, so there is no tolerance.  Inputs carry NaN in every pixel
no patch covers and lie inside a NaN-filled buffer, at an aligned base (k = 0: the wide loads where the geometry allows
them) and 4 bytes off (k = 1: the dword path, picked from the pointer)."""

import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from view_cases import FUSED, FUSED_ROUND, GENERIC, POOL50, POOL50_CUT, POOL100, geom_id, grid, guarded_images

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_NETS = {}


def net_for(kind, **over):
    """One net per configuration for the whole module (weights packed once)."""
    key = (kind, tuple(sorted(over.items())))
    if key not in _NETS:
        conf = {"mnist": lambda: synth.mnist_conf(**over),
                "mnist50": lambda: synth.mnist_conf(patch=50, **over),
                "traffic": lambda: synth.traffic_conf(**over),
                "generic": lambda: synth.traffic_conf(patch=37, **over)}[kind]()
        if kind == "generic":
            conf = conf.clone(patch_size=[37, 45], patch_stride=[37, 45])
        _NETS[key] = synth.fill_weights(IPSNet(DEV, conf), 5).to(DEV).eval()
    return _NETS[key]


def plan_of(net):
    return net.selection.plan()


def check_geometry(net, g, name, firsts=()):
    b, c, h, w, patch, stride = g
    plan = plan_of(net)
    ny, nx = grid(g)
    for k in (0, 1):
        images = guarded_images(g, k, device=DEV)
        assert images.data_ptr() % 16 == 4 * k
        view = hip.PatchView(images.shape, patch, stride)
        assert plan.view_supported(view) and plan.view_kernel_name(view) == name
        patches = hip.patchify(images, patch, stride)
        assert bool(torch.isfinite(patches).all())
        flat = patches.reshape(-1, *patches.shape[2:])
        want = plan.encode(flat)
        got = plan.encode_view(images, view)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
        perm = torch.randperm(view.count, generator=torch.Generator().manual_seed(3 + k)).to(DEV)
        assert torch.equal(plan.encode_view(images, view, index=perm.to(torch.int32)), want[perm])
        for first, n in firsts:
            assert torch.equal(plan.encode_view(images, view, first=first, n=n), want[first:first + n])
        m = min(7, view.per_image)
        idx = torch.stack([torch.randperm(view.per_image, generator=torch.Generator().manual_seed(9 + i))[:m] for i in range(b)]).to(DEV)
        rows = hip.gather_patches_view(images, view, idx)
        assert torch.equal(rows, hip.gather_rows(patches, idx))
        for bi in range(b):
            for j in range(m):
                py, px = divmod(int(idx[bi, j]), nx)
                y0, x0 = py * stride[0], px * stride[1]
                assert torch.equal(rows[bi, j], images[bi, :, y0:y0 + patch[0], x0:x0 + patch[1]])
    torch.cuda.synchronize()


@pytest.mark.parametrize("g", FUSED, ids=geom_id)
def test_fused_trunk_reads_the_grid(g):
    check_geometry(net_for("mnist", N=64, M=8, I=8), g, "fused_trunk_view_kernel")


def test_fused_trunk_a_whole_round_and_the_pair_remainder():
    cus = hip.device_geometry(DEV).cus
    ny, nx = grid(FUSED_ROUND)
    assert ny * nx >= 8 * cus + 5, "the shape is meant to fill one whole round of the eight-patch kernel and leave a remainder"
    check_geometry(net_for("mnist", N=64, M=8, I=8), FUSED_ROUND, "fused_trunk_view_kernel", firsts=[(3, 1), (8 * cus - 3, 11)])


@pytest.mark.parametrize("g", POOL50, ids=geom_id)
def test_stem_pool50_reads_the_grid(g):
    check_geometry(net_for("mnist50", N=64, M=8, I=8), g, "stem_pool50_view_kernel", firsts=[(0, 1), (1, 4), (2, 5), (3, 9)])


def test_stem_pool50_across_the_two_stream_cut():
    check_geometry(net_for("mnist50", N=64, M=8, I=8), POOL50_CUT, "stem_pool50_view_kernel", firsts=[(1023, 9)])


@pytest.mark.parametrize("g", POOL100, ids=geom_id)
def test_stem_pool100x3_reads_the_grid(g):
    check_geometry(net_for("traffic", N=48, M=16, I=32), g, "stem_pool100x3_view_kernel", firsts=[(1, 3)])


# ---------------------------------------------------------------- ips_image against ips(patchify)
def run_both(net, images, patch, stride, seed=None, view_expected=True, host=False):
    sel = net.selection
    if seed is not None:
        torch.manual_seed(seed)
    want = net.ips(hip.patchify(images, patch, stride))
    want += (net.last_mem_idx, net.last_mem_emb, net.last_shuffle)
    want = [None if t is None else t.clone() for t in want]
    before = (sel.view_calls, sel.index_calls)
    if seed is not None:
        torch.manual_seed(seed)
    got = net.ips_image(images.cpu() if host else images, patch, stride)
    got += (net.last_mem_idx, net.last_mem_emb, net.last_shuffle)
    torch.cuda.synchronize()
    assert sel.view_calls - before[0] == (1 if view_expected else 0)
    for name, a, b in zip(("mem_patch", "mem_pos", "last_mem_idx", "last_mem_emb", "last_shuffle"), got, want):
        assert (a is None) == (b is None), name
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), name
    return sel.index_calls - before[1]


def normal_images(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_ips_image_mnist_16_images_parts_in_one_launch():
    net = net_for("mnist", N=2500)
    run_both(net, normal_images((16, 1, 1600, 1600), 1), (32, 32), (32, 32))


@pytest.mark.parametrize("style", ["batch", "instance"])
def test_ips_image_shuffled_through_the_index(style):
    net = net_for("mnist", N=2500, shuffle=True, shuffle_style=style)
    assert run_both(net, normal_images((16, 1, 1600, 1600), 2), (32, 32), (32, 32), seed=21) == 1      # (ips_image: through the index)
    assert net.last_shuffle is not None


def test_ips_image_mnist_small_batch():
    run_both(net_for("mnist", N=300, M=16, I=16), normal_images((2, 1, 480, 640), 3), (32, 32), (32, 32))


def test_ips_image_one_image_takes_the_parts():
    net = net_for("mnist", N=2500)
    run_both(net, normal_images((1, 1, 1600, 1600), 4), (32, 32), (32, 32))


def test_ips_image_one_image_at_stride_8():
    run_both(net_for("mnist", N=2116), normal_images((1, 1, 392, 392), 5), (32, 32), (8, 8))


def test_ips_image_mnist50_ragged_last_chunk():
    run_both(net_for("mnist50", N=196, M=32, I=48), normal_images((2, 1, 700, 700), 6), (50, 50), (50, 50))


def test_ips_image_mnist50_long_loop_parts_through_index_lists():
    """961 overlapping 50-px patches, M = I = 8: 120 iterations - a layer-by-layer trunk whose parts are index lists."""
    net = net_for("mnist50", N=961, M=8, I=8)
    run_both(net, normal_images((1, 1, 800, 800), 7), (50, 50), (25, 25))
    net = net_for("mnist50", N=961, M=8, I=8, shuffle=True, shuffle_style="instance")
    run_both(net, normal_images((1, 1, 800, 800), 7), (50, 50), (25, 25), seed=5)


def test_ips_image_traffic():
    run_both(net_for("traffic", N=48, M=16, I=32), normal_images((2, 3, 600, 800), 8), (100, 100), (100, 100))


def test_ips_image_host_images_give_the_device_result():
    run_both(net_for("mnist", N=300, M=16, I=16), normal_images((2, 1, 480, 640), 9), (32, 32), (32, 32), host=True)


def test_generic_stem_materialises_the_patches():
    net = net_for("generic", N=9, M=4, I=2)
    b, c, h, w, patch, stride = GENERIC
    images = guarded_images(GENERIC, 0, device=DEV)
    assert not plan_of(net).view_supported(hip.PatchView(images.shape, patch, stride))
    assert plan_of(net).view_kernel_name(hip.PatchView(images.shape, patch, stride)) is None
    run_both(net, images, patch, stride, view_expected=False)


def test_the_patch_tensor_is_not_allocated():
    """B = 4 images of 392x392 at stride 8: the patch tensor would be 4 x 2,116 x 4 KiB = 34.7 MB; the call's own buffers
    (embeddings 4.3 MB, logits <= 1.1 MB, indices) stay under 6 MB - half the tensor's bytes is only reached by making it."""
    net = net_for("mnist", N=2116)
    images = normal_images((4, 1, 392, 392), 10)
    net.ips_image(images, (32, 32), (8, 8))                    # warmed: weights packed, the pipelines' buffers exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.max_memory_allocated(DEV)
    out = net.ips_image(images, (32, 32), (8, 8))
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated(DEV) - base
    tensor_bytes = 4 * 2116 * 32 * 32 * 4
    print("peak above the input: %.2f MB (patch tensor %.2f MB)" % (used / 1e6, tensor_bytes / 1e6))
    assert out[0].shape == (4, 64, 1, 32, 32)
    assert used < tensor_bytes // 2


# ---------------------------------------------------------------- refusals
def test_uint8_images_raise():
    net = net_for("mnist", N=300, M=16, I=16)
    with pytest.raises(TypeError, match="dequantisation table"):
        net.ips_image(torch.zeros((2, 1, 480, 640), dtype=torch.uint8, device=DEV), (32, 32), (32, 32))


def test_bf16_precision_falls_back_to_the_patch_tensor(monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=300, M=16, I=16)), 5).to(DEV).eval()
    images = normal_images((2, 1, 480, 640), 11)
    assert not plan_of(net).view_supported(hip.PatchView(images.shape, (32, 32), (32, 32)))
    run_both(net, images, (32, 32), (32, 32), view_expected=False)
