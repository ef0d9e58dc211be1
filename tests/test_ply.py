"""nerf_pl_amd.extract.write_ply: the binary little-endian PLY that
extract_color_mesh.py:286-297 writes through plyfile, read back with the small
reader of tests/mesh_ref.py."""
import numpy as np
import pytest
import torch

import mesh_ref as R

HEAD = ["ply", "format binary_little_endian 1.0", "element vertex 5", "property float x",
        "property float y", "property float z"]
COLOUR = ["property uchar red", "property uchar green", "property uchar blue"]
TAIL = ["element face 3", "property list uchar int vertex_indices", "end_header"]


def _mesh():
    g = np.random.Generator(np.random.PCG64(3))
    v = g.standard_normal((5, 3)).astype(np.float32)
    v[0, 0] = np.float32(1e-30)
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 0, 1]], dtype=np.int32)
    c = g.integers(0, 256, size=(5, 3)).astype(np.uint8)
    return v, t, c


def test_ply_without_colours(tmp_path):
    from nerf_pl_amd.extract import write_ply
    v, t, _ = _mesh()
    p = tmp_path / "m.ply"
    write_ply(p, v, t)
    header, v2, c2, t2 = R.read_ply(p)
    assert header == HEAD + TAIL
    assert c2 is None
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(t2, t)
    assert p.stat().st_size == len("\n".join(header)) + 1 + 5 * 12 + 3 * 13


def test_ply_with_colours_from_tensors(tmp_path):
    from nerf_pl_amd.extract import write_ply
    v, t, c = _mesh()
    p = tmp_path / "m.ply"
    write_ply(str(p), torch.from_numpy(v), torch.from_numpy(t), torch.from_numpy(c))
    header, v2, c2, t2 = R.read_ply(p)
    assert header == HEAD + COLOUR + TAIL
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(c2, c)
    np.testing.assert_array_equal(t2, t)
    assert p.stat().st_size == len("\n".join(header)) + 1 + 5 * 15 + 3 * 13


def test_ply_empty_mesh_and_colour_count(tmp_path):
    from nerf_pl_amd.extract import write_ply
    p = tmp_path / "e.ply"
    write_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    header, v2, _, t2 = R.read_ply(p)
    assert "element vertex 0" in header and "element face 0" in header
    assert v2.shape == (0, 3) and t2.shape == (0, 3)
    v, t, c = _mesh()
    with pytest.raises(ValueError):
        write_ply(p, v, t, c[:4])
