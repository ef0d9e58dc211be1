"""nerf_pl_amd.extract.write_ply with vertex normals: ``nx ny nz`` as float
after ``x y z`` and before the colours, parsed here from the bytes; without
normals the file is byte for byte what the writer produced before it knew
about them."""
import struct

import numpy as np
import pytest
import torch

HEAD = ["ply", "format binary_little_endian 1.0", "element vertex 5", "property float x",
        "property float y", "property float z"]
NORMAL = ["property float nx", "property float ny", "property float nz"]
COLOUR = ["property uchar red", "property uchar green", "property uchar blue"]
TAIL = ["element face 3", "property list uchar int vertex_indices", "end_header"]


def _mesh():
    g = np.random.Generator(np.random.PCG64(5))
    v = g.standard_normal((5, 3)).astype(np.float32)
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 0, 1]], dtype=np.int32)
    c = g.integers(0, 256, size=(5, 3)).astype(np.uint8)
    n = g.standard_normal((5, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[0] = (0.0, 0.0, 1.0)
    return v, t, c, n


def _parse(raw):
    """(header lines, {property: column}, triangles): the vertex element's
    properties in header order, float -> <f4 and uchar -> u1"""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    nv = int([h for h in header if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in header if h.startswith("element face")][0].split()[-1])
    lo = header.index([h for h in header if h.startswith("element vertex")][0])
    hi = header.index([h for h in header if h.startswith("element face")][0])
    fields = [(h.split()[2], {"float": "<f4", "uchar": "u1"}[h.split()[1]])
              for h in header[lo + 1:hi]]
    vt = np.dtype(fields)
    assert vt.itemsize == sum(np.dtype(f[1]).itemsize for f in fields)      # packed
    ft = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
    assert len(raw) == end + nv * vt.itemsize + nf * ft.itemsize
    v = np.frombuffer(raw, vt, nv, end)
    f = np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    assert (f["n"] == 3).all()
    return header, {name: v[name] for name, _ in fields}, f["idx"].copy()


@pytest.mark.parametrize("with_colours", [False, True])
def test_ply_round_trip_with_normals(tmp_path, with_colours):
    from nerf_pl_amd.extract import write_ply
    v, t, c, n = _mesh()
    p = tmp_path / "m.ply"
    # float64 normals (what vertex_normals returns) as a tensor, the rest as arrays
    write_ply(p, v, t, c if with_colours else None, normals=torch.from_numpy(n))
    header, cols, t2 = _parse(p.read_bytes())
    assert header == HEAD + NORMAL + (COLOUR if with_colours else []) + TAIL
    assert list(cols) == ["x", "y", "z", "nx", "ny", "nz"] + \
        (["red", "green", "blue"] if with_colours else [])
    np.testing.assert_array_equal(np.stack([cols[k] for k in "xyz"], 1), v)
    np.testing.assert_array_equal(np.stack([cols[k] for k in ("nx", "ny", "nz")], 1),
                                  n.astype(np.float32))
    if with_colours:
        np.testing.assert_array_equal(np.stack([cols[k] for k in ("red", "green", "blue")], 1), c)
    np.testing.assert_array_equal(t2, t)
    assert p.stat().st_size == len("\n".join(header)) + 1 + 5 * (24 + 3 * with_colours) + 3 * 13


@pytest.mark.parametrize("with_colours", [False, True])
def test_ply_without_normals_keeps_its_bytes(tmp_path, with_colours):
    """the bytes spelled out by hand: header, packed vertex records, faces"""
    from nerf_pl_amd.extract import write_ply
    v, t, c, _ = _mesh()
    want = ("\n".join(HEAD + (COLOUR if with_colours else []) + TAIL) + "\n").encode("ascii")
    for k in range(5):
        want += struct.pack("<3f", *v[k].tolist())
        if with_colours:
            want += struct.pack("<3B", *c[k].tolist())
    for tri in t.tolist():
        want += struct.pack("<B3i", 3, *tri)
    a, b = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(a, v, t, c if with_colours else None)
    write_ply(b, v, t, c if with_colours else None, None)
    assert a.read_bytes() == want and b.read_bytes() == want


def test_ply_normal_count(tmp_path):
    from nerf_pl_amd.extract import write_ply
    v, t, c, n = _mesh()
    with pytest.raises(ValueError, match="normals"):
        write_ply(tmp_path / "e.ply", v, t, c, n[:4])
