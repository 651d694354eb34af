"""The training-step feature projector (csrc/projector_train.hip, training/fused_projector.py): what can be checked without
a GPU - the library exports and the header declares the new entry points, and ``supported`` accepts exactly the
reference's projector."""

import ctypes
import os

import pytest
import torch
from torch import nn

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.training import fused_projector

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ipsx_projector_train_supported", "ipsx_projector_train_slabs", "ipsx_projector_train_forward",
       "ipsx_projector_wgrad_chunk_rows", "ipsx_projector_wgrad_max_rows", "ipsx_projector_wgrad_workspace_bytes", "ipsx_projector_wgrad")


def test_library_exports_the_training_projector():
    so = ctypes.CDLL(hip.library_path())
    for name in NEW:
        assert hasattr(so, name), name
    lib = hip.lib()
    assert lib.ipsx_version() >= 304 and lib.ipsx_version() // 100 == hip.ABI_MAJOR
    chunk = lib.ipsx_projector_wgrad_chunk_rows()
    assert chunk > 0 and chunk % 2 == 0
    for dtype, size in ((0, 4), (1, 2), (2, 2)):
        rows = lib.ipsx_projector_wgrad_max_rows(2048, 512, dtype)
        assert rows % chunk == 0 and rows * 2048 * size < 1 << 31 and (rows + chunk) * 2048 * size >= (1 << 31) - (1 << 20)
    assert lib.ipsx_projector_wgrad_workspace_bytes(80000, 2048, 512) == -(-80000 // chunk) * (512 * 2048 + 512) * 4
    assert lib.ipsx_projector_train_slabs(80000) == 1250 and lib.ipsx_projector_train_slabs(65) == 2


def test_header_declares_the_training_projector():
    text = open(os.path.join(REPO, "include", "ipsx.h")).read()
    for name in NEW:
        assert name + "(" in text, name


def _projector(f=2048, d=512, **over):
    ln = over.get("ln", nn.LayerNorm(f, eps=1e-5, elementwise_affine=False))
    lin = over.get("lin", nn.Linear(f, d))
    bn = over.get("bn", nn.BatchNorm1d(d))
    return nn.Sequential(ln, lin, bn, over.get("act", nn.ReLU()))


def test_supported_accepts_the_reference_projector():
    assert fused_projector.supported(_projector())
    net = IPSNet(torch.device("cpu"), synth.camelyon_conf(N=64, M=8, I=8))
    assert fused_projector.supported(net.encoder)
    assert fused_projector.supported(_projector(64, 32)) and fused_projector.supported(_projector(512, 128))
    assert fused_projector.enabled()


@pytest.mark.parametrize("case", ["ln_affine", "no_bias", "no_running_stats", "f_100", "f_2056", "d_192", "d_16", "d_2048",
                                  "momentum_none", "bn_no_affine", "gelu", "three_modules", "image_trunk"])
def test_supported_refuses(case):
    enc = {
        "ln_affine": lambda: _projector(ln=nn.LayerNorm(2048)),
        "no_bias": lambda: _projector(lin=nn.Linear(2048, 512, bias=False)),
        "no_running_stats": lambda: _projector(bn=nn.BatchNorm1d(512, track_running_stats=False)),
        "f_100": lambda: _projector(100, 512),
        "f_2056": lambda: _projector(2056, 512),
        "d_192": lambda: _projector(2048, 192),
        "d_16": lambda: _projector(2048, 16),
        "d_2048": lambda: _projector(2048, 2048),
        "momentum_none": lambda: _projector(bn=nn.BatchNorm1d(512, momentum=None)),
        "bn_no_affine": lambda: _projector(bn=nn.BatchNorm1d(512, affine=False)),
        "gelu": lambda: _projector(act=nn.GELU()),
        "three_modules": lambda: nn.Sequential(nn.LayerNorm(2048, elementwise_affine=False), nn.Linear(2048, 512), nn.ReLU()),
        "image_trunk": lambda: IPSNet(torch.device("cpu"), synth.mnist_conf(N=16, M=4, I=4)).encoder,
    }[case]()
    assert not fused_projector.supported(enc)


def test_switch(monkeypatch):
    monkeypatch.setenv("IPSX_TRAIN_PROJECTOR", "0")
    assert not fused_projector.enabled()
    monkeypatch.setenv("IPSX_TRAIN_PROJECTOR", "1")
    assert fused_projector.enabled()
