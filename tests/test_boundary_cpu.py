"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every
symbol include/pointnet_refine_hip.h declares, the nn.Module surface has the reference's
state_dict (G6 manifest), a strict load of a reference-shaped checkpoint works, and the
product path refuses CPU tensors instead of silently falling back."""
import ctypes
import json
import os
import re

import pytest
import torch

from oracle import procedural as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from pointnet_refine_amd import _lib
    _lib.build()
    return _lib


def test_library_exports_header_symbols(built):
    hdr = open(os.path.join(ROOT, "include", "pointnet_refine_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(prh_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 14
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert sorted(built.EXPORTS) == declared
    assert b"gfx950" in built.lib().prh_version()


def test_workspace_queries_are_pure(built):
    lib = built.lib()
    a = lib.prh_encoder_workspace_bytes(8, 256, 4, 1024, 0)
    b = lib.prh_encoder_workspace_bytes(8, 256, 4, 1024, 1)
    assert 0 < a < b
    # backward scratch is dominated by dy_cat [P,1984] fp32
    assert b > 8 * 256 * 1984 * 4
    assert lib.prh_linear_backward_workspace_bytes(2048, 1024, 256) > 1024 * 256 * 4


def test_state_dict_matches_reference_manifest(golden_dir):
    from pointnet_refine_amd.model import LineRefineNet
    man = json.load(open(os.path.join(golden_dir, "g6_state_dict_manifest.json")))
    m = LineRefineNet()
    ours = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]
    assert ours == man["entries"]
    assert sum(p.numel() for p in m.parameters()) == man["n_params"]
    res = m.load_state_dict(P.linerefine_state_dict(0), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_constructor_signatures():
    import inspect
    from pointnet_refine_amd import model as M
    assert str(inspect.signature(M.LineRefineNet.__init__)) == "(self, num_line_points=32, feature_dim=1024)"
    assert str(inspect.signature(M.MultiScalePointNetEncoder.__init__)) == "(self, in_channel=4, out_dim=1024)"
    assert str(inspect.signature(M.PositionalEncoding.__init__)) == "(self, in_dim=3, out_dim=256)"
    assert str(inspect.signature(M.DetrTransformerDecoderLayer.__init__)) == \
        "(self, d_model=256, nhead=8, dim_feedforward=1024, dropout=0.1)"
    enc = M.MultiScalePointNetEncoder(in_channel=6, out_dim=1024)
    assert enc.conv1.weight.shape == (64, 6, 1)


def test_no_cpu_fallback(built):
    from pointnet_refine_amd.model import LineRefineNet
    m = LineRefineNet().eval()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        m(torch.randn(2, 64, 4), torch.randn(2, 32, 3))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "pointnet_refine_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f


def test_environment_switches_match_integration_table():
    """Every PRH_* variable the library (getenv in csrc/) or the package (os.environ) reads has a row in
    INTEGRATION.md section 6, and every PRH_* row there is read somewhere."""
    pkg = os.path.join(ROOT, "pointnet_refine_amd")
    read = set()
    for f in os.listdir(os.path.join(pkg, "csrc")):
        read |= set(re.findall(r'getenv\(\s*"(PRH_\w+)"', open(os.path.join(pkg, "csrc", f)).read()))
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            txt = open(os.path.join(pkg, f)).read()
            read |= set(re.findall(r'os\.(?:environ\.get\(|environ\[|getenv\()\s*"(PRH_\w+)"', txt))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = re.search(r"^## 6\..*?(?=^## |\Z)", doc, flags=re.S | re.M).group(0)
    listed = set(re.findall(r"^\| `(PRH_\w+)", sec, flags=re.M))
    assert read == listed, f"read but not listed: {sorted(read - listed)}; listed but not read: {sorted(listed - read)}"
