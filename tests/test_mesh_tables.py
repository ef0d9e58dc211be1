"""The crack-free certificate of nerf_pl_amd.mesh_tables.MC_TRI_TABLE: all 256
cases, no field.  A case's triangles may only meet the cube's faces in
segments that depend on that face's four corner bits alone, so that the two
cells sharing a face always draw the same segments there; inside the cube the
triangles must close up."""
import itertools

import numpy as np
import pytest

from nerf_pl_amd.mesh_tables import MC_CORNERS, MC_EDGE_CORNERS, MC_ROW, MC_TRI_TABLE

FACES = [(a, s) for a in range(3) for s in range(2)]


def _on_face(e, face):
    a, s = face
    return all(MC_CORNERS[c][a] == s for c in MC_EDGE_CORNERS[e])


def _common_face(e1, e2):
    f = [face for face in FACES if _on_face(e1, face) and _on_face(e2, face)]
    assert len(f) <= 1
    return f[0] if f else None


def _triangles(case):
    row = MC_TRI_TABLE[case]
    n = row.index(-1)
    assert n % 3 == 0 and all(x == -1 for x in row[n:]) and all(0 <= x < 12 for x in row[:n])
    return [row[i:i + 3] for i in range(0, n, 3)]


def _directed(case):
    c = {}
    for t in _triangles(case):
        assert len(set(t)) == 3
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            c[(a, b)] = c.get((a, b), 0) + 1
    return c


def _face_segments(case, face):
    return {(a, b) for (a, b) in _directed(case) if _on_face(a, face) and _on_face(b, face)}


def _bit(case, corner):
    return (case >> corner) & 1


def _midpoint(e):
    return np.mean([MC_CORNERS[c] for c in MC_EDGE_CORNERS[e]], axis=0)


def test_table_shape_and_conventions():
    assert len(MC_TRI_TABLE) == 256 and all(len(r) == MC_ROW == 16 for r in MC_TRI_TABLE)
    assert [tuple(c) for c in MC_CORNERS] == [(b & 1, b >> 1 & 1, b >> 2 & 1) for b in range(8)]
    for e, (c0, c1) in enumerate(MC_EDGE_CORNERS):
        a = e // 4
        others = [x for x in range(3) if x != a]
        d = np.subtract(MC_CORNERS[c1], MC_CORNERS[c0])
        assert d[a] == 1 and d[others[0]] == 0 and d[others[1]] == 0 and MC_CORNERS[c0][a] == 0
        assert MC_CORNERS[c0][others[0]] + 2 * MC_CORNERS[c0][others[1]] == e % 4


def test_empty_cases():
    """(d) nothing to draw when every corner is on one side"""
    assert _triangles(0) == [] and _triangles(255) == []


@pytest.mark.parametrize("case", range(256))
def test_case_is_closed_inside_and_uses_crossed_edges(case):
    """(a) a triangle edge inside one cube face is a boundary segment and
    occurs exactly once; every other triangle edge is interior and occurs
    exactly twice, once in each direction.  The vertices used are exactly the
    cube edges whose corner bits differ."""
    c = _directed(case)
    crossed = {e for e, (c0, c1) in enumerate(MC_EDGE_CORNERS) if _bit(case, c0) != _bit(case, c1)}
    assert {e for pair in c for e in pair} == crossed
    for (a, b), n in c.items():
        if _common_face(a, b) is not None:
            assert n == 1 and (b, a) not in c, (case, a, b)
        else:
            assert n == 1 and c.get((b, a), 0) == 1, (case, a, b)


def _across(e, axis):
    """the cube edge opposite ``e`` (which lies on face (axis, 0)) on face (axis, 1)"""
    want = []
    for c in MC_EDGE_CORNERS[e]:
        p = list(MC_CORNERS[c])
        assert p[axis] == 0
        p[axis] = 1
        want.append(tuple(p))
    for e2, cs in enumerate(MC_EDGE_CORNERS):
        if [tuple(MC_CORNERS[c]) for c in cs] == want:
            return e2
    raise AssertionError(e)


@pytest.mark.parametrize("axis", range(3))
def test_neighbours_agree_on_the_shared_face(axis):
    """(b) for each of the 16 patterns of a face's four corner bits, every case
    showing it on face (axis, 1), and every case showing it on face (axis, 0)
    -- which is the same face seen from the neighbour, so its segments are
    mapped across and reversed -- draws the same set of segments."""
    others = [x for x in range(3) if x != axis]
    seen = {}
    for case in range(256):
        for side in (0, 1):
            pattern = 0
            for c, p in enumerate(MC_CORNERS):
                if p[axis] == side:
                    pattern |= _bit(case, c) << (p[others[0]] + 2 * p[others[1]])
            segs = _face_segments(case, (axis, side))
            if side == 0:
                segs = {(_across(b, axis), _across(a, axis)) for a, b in segs}
            seen.setdefault(pattern, set()).add(frozenset(segs))
    assert sorted(seen) == list(range(16))
    for pattern, variants in seen.items():
        assert len(variants) == 1, (axis, pattern, variants)
        n_cross = sum(((pattern >> i) & 1) != ((pattern >> j) & 1)
                      for i, j in ((0, 1), (1, 3), (3, 2), (2, 0)))
        assert len(next(iter(variants))) == n_cross // 2


@pytest.mark.parametrize("case", range(256))
def test_segments_keep_the_occupied_corner_on_the_right(case):
    """(c) seen from outside the cube, each face segment runs with the empty
    corner (bit set, sigma < thr) of both cube edges it joins on its left and
    their occupied corner (sigma >= thr) on its right: the triangle normals
    point from the occupied side to the empty side."""
    for face in FACES:
        a, s = face
        normal = np.zeros(3)
        normal[a] = 1.0 if s else -1.0
        for e1, e2 in _face_segments(case, face):
            m1, m2 = _midpoint(e1), _midpoint(e2)
            left = np.cross(normal, m2 - m1)
            for e in (e1, e2):
                for c in MC_EDGE_CORNERS[e]:
                    side = float(np.dot(left, np.asarray(MC_CORNERS[c], dtype=float) - m1))
                    assert side != 0
                    assert (side > 0) == bool(_bit(case, c)), (case, face, e1, e2, c)


def test_every_boundary_segment_lies_on_a_face_edge_pair():
    """the boundary of each case (edges used once) is exactly the union of its face segments"""
    for case in range(256):
        c = _directed(case)
        boundary = {(a, b) for (a, b) in c if (b, a) not in c}
        on_faces = set(itertools.chain.from_iterable(_face_segments(case, f) for f in FACES))
        assert boundary == on_faces
