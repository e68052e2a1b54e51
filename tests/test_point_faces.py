"""The two faces of every point-set operation (fi_<op> over a context, fi_points_<op> over a point set) on a machine
without a GPU: a null handle is refused with FI_ERR_INVALID and the face's own sentence before any device is touched, and
the table the tests of the two faces share (point_faces.py) names exactly the pairs the ctypes mirror declares."""
import ctypes as C

import pytest

import point_faces as P


def test_the_table_names_every_pair_the_mirror_declares():
    from field_interpolation_amd import _capi
    names = set(_capi.SYMBOLS)
    pairs = {s[len(P.SET_FACE):] for s in names if s.startswith(P.SET_FACE) and P.CONTEXT_FACE + s[len(P.SET_FACE):] in names}
    assert pairs == set(P.OPS)
    assert len(P.OPS) == 11


@pytest.mark.parametrize("op", P.OPS)
@pytest.mark.parametrize("face, text", [(P.CONTEXT_FACE, "null context"), (P.SET_FACE, "point set is null")])
def test_a_null_handle_is_refused(op, face, text):
    assert P.call(face, op, C.c_void_p(), P.Buffers(3, 8, 4, [4, 4, 4])) == (1, text)
