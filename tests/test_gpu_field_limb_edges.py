"""The field arithmetic of snarkvm_amd/csrc/ff.hip.h and the square roots of serde.hip.h as gfx950 compiles them, on operands chosen as
internal 29-bit limb patterns: the cases of tests/test_field_limb_edges_host.py through snarkvm_hip_devtest_field / _field_ext (one thread per
case), and the compressed-point decoder on the curve points whose y comes out of the square root's early returns: (0, +-1) and (-1, 0)."""
import pytest

from oracle import pyref
from snarkvm_amd import serialize
from tests import util
from tests.helpers import field_edge_checks as fc

pytestmark = pytest.mark.gpu

RUN = fc.Runner(device=True)
Q = pyref.Q_MOD


@pytest.mark.parametrize("field", [0, 1])
def test_binary_ops_on_every_ordered_pair(field):
    fc.check_binary_ops(RUN, field)


@pytest.mark.parametrize("field", [0, 1])
def test_add_sub_neg_dbl_mul_leave_canonical_internal_limbs(field):
    fc.check_raw_internal_limbs(RUN, field)


@pytest.mark.parametrize("field", [0, 1])
def test_unary_ops_on_every_element(field):
    fc.check_unary_ops(RUN, field)


@pytest.mark.parametrize("field", [0, 1])
def test_diff_of_products_four_operands_all_correction_branches(field):
    fc.check_diff_of_products(RUN, field)


def test_fq2_mul_sqr_inverse_diff_of_products():
    fc.check_fq2(RUN)


def test_fq_sqrt_every_two_adic_order(golden):
    fc.check_fq_sqrt(RUN, golden)


def test_fq2_sqrt_every_branch():
    fc.check_fq2_sqrt(RUN)


def _enc(x, positive):
    b = bytearray(x.to_bytes(48, "little"))
    b[47] |= (1 << 7) if positive else 0
    return bytes(b)


# (x, sign flag) -> point: x = 0 has y^2 = 1 (a^T == 1: no Tonelli-Shanks round), x = q - 1 has y^2 = 0 (fq_sqrt's early return, y == -y)
SPECIAL = [((0, False), (0, 1)), ((0, True), (0, Q - 1)), ((Q - 1, False), (Q - 1, 0)), ((Q - 1, True), (Q - 1, 0))]


def test_decoder_on_points_of_order_two_and_three():
    for (x, pos), want in SPECIAL:
        enc = _enc(x, pos)
        assert pyref.g1_deserialize(enc, compressed=True) == want
        assert util.g1_affine_to_ints(serialize.g1_deserialize(enc, compressed=True)) == [want], (x, pos)
        with pytest.raises(serialize.SerializationError):  # order 3 / order 2: on the curve, outside the prime-order subgroup
            serialize.g1_deserialize(enc, compressed=True, validate=True)


def test_decoder_special_record_inside_a_batch(golden):
    """the status word is one per batch: the only bad record, 300 of 600, is decoded by a workgroup in the middle of the grid (64 records each), so
    the word is set from a workgroup that is neither the first nor the last"""
    pts = util.srs_points_ints(golden["srs_g1"], 600)
    good = [pyref.g1_serialize(p, True) for p in pts]
    assert util.g1_affine_to_ints(serialize.g1_deserialize(b"".join(good), compressed=True, validate=True)) == pts
    for (x, pos), want in SPECIAL:
        recs = list(good)
        recs[300] = _enc(x, pos)
        data = b"".join(recs)
        got = util.g1_affine_to_ints(serialize.g1_deserialize(data, compressed=True))
        assert got == pts[:300] + [want] + pts[301:], (x, pos)
        with pytest.raises(serialize.SerializationError):
            serialize.g1_deserialize(data, compressed=True, validate=True)
