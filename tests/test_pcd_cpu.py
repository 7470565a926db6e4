"""PCD codec, host side: the header helpers against drive.write_scene's header, and the refusal to
run the device functions without a GPU.  The codec itself is tested in test_pcd_gpu.py."""
import numpy as np
import pytest
import torch


def test_module_imports_and_hostfallback_is_a_valueerror():
    from pointnet_refine_amd import pcd
    assert issubclass(pcd.HostFallback, ValueError)
    e = pcd.HostFallback("format_rows", 70)
    assert e.row == 70 and "row 70" in str(e)
    for name in ("format_rows", "parse_rows", "write_pcds", "write_pcd", "read_pcd"):
        assert callable(getattr(pcd, name))


@pytest.mark.parametrize("n", [0, 1, 12345])
def test_header_matches_write_scene(tmp_path, n):
    from pointnet_refine_amd import drive, pcd
    pts = np.arange(4.0 * n).reshape(n, 4)
    path = str(tmp_path / "s.pcd")
    drive.write_scene(path, str(tmp_path / "s.json"), pts, [], "t")
    data = open(path, "rb").read()
    hdr = pcd.header_bytes(n)
    assert data[:len(hdr)] == hdr and hdr.count(b"\n") == 10
    if n == 0:
        assert data == hdr
    info = pcd.parse_header(bytearray(data))
    assert info["length"] == len(hdr) and info["lines"] == 10 and info["points"] == n
    assert info["data"] == b"ascii" and info["fields"] == [b"x", b"y", b"z", b"intensity"]


def test_parse_header_binary_and_bad():
    from pointnet_refine_amd import pcd
    raw = b"# .PCD v0.7\r\nFIELDS x y z intensity\r\nPOINTS 3\r\nDATA binary\r\n" + b"\x00" * 42
    info = pcd.parse_header(raw)
    assert info["data"] == b"binary" and info["points"] == 3 and len(raw) - info["length"] == 42
    assert info["lines"] == 4
    with pytest.raises(ValueError, match="DATA"):
        pcd.parse_header(b"VERSION 0.7\nFIELDS x y z\n")
    with pytest.raises(ValueError, match="DATA"):
        pcd.parse_header(b"")


def test_pcd_refuses_to_run_without_gpu(monkeypatch, tmp_path):
    from pointnet_refine_amd import pcd
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        pcd.format_rows(np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match="GPU"):
        pcd.parse_rows(b"1 2 3 4\n", 4)
    with pytest.raises(RuntimeError, match="GPU"):
        pcd.read_pcd(str(tmp_path / "missing.pcd"))
    with pytest.raises(RuntimeError, match="GPU"):
        pcd.write_pcd(str(tmp_path / "a.pcd"), np.zeros((3, 4)), strict=True)
