"""The bits of the trainable-condition kernels (csrc/cond_bag.h, cond_csr.h; cond_bits_cases.py): aae_cat_* against aae_bag_*
at padding row 0 bit for bit, and every call family against the digests recorded in tests/golden/cond_bits.json."""
import json

import numpy as np
import pytest

import bag_cases as BC
import cond_bits_cases as CB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sparse", [False, True], ids=["adam", "sparse_adam"])
@pytest.mark.parametrize("reduce", [BC.SUM, BC.MEAN_WIDTH], ids=["sum", "mean"])
def test_cat_equals_bag_at_padding_row_0_bit_for_bit(reduce, sparse):
    """cat_encode / cat_update(mean=False | True) against bag_encode / bag_update(BAG_SUM | BAG_MEAN_WIDTH, padding_idx=0) -
    the distinct entry points aae_cat_* and aae_bag_* - over rows {1, 3, 65} x dim {1, 7, 64, 65, 256} x vocab {2, 40} on
    off-grid tables and gradients and ragged_cases.make_lists' lists padded with 0 (the empty and the all-out-of-vocabulary
    list, one table row three times in a list and in two others, the indices -3, vocab and 2^30): the encoded blocks, the table
    and both moments after each of two consecutive steps, so non-zero moments enter the second."""
    for rows in (1, 3, 65):
        for dim in (1, 7, 64, 65, 256):
            for vocab in (2, 40):
                table, lists, douts, _ = CB.make_inputs(10 * reduce + rows + dim + vocab, rows, dim, vocab, 0)
                if rows == 65:
                    flat = [j for row in lists for j in row]
                    assert [] in lists and [vocab, -3, 2 ** 30] in lists and -3 in flat and 2 ** 30 in flat
                    assert lists[3].count(lists[3][0]) >= 3 and lists[3][0] in lists[5] and lists[3][0] in lists[7]
                for steps in (1, 2):
                    cat = CB.run("cat", table, lists, douts[:steps], reduce, 0, sparse)
                    bag = CB.run("bag", table, lists, douts[:steps], reduce, 0, sparse)
                    for name, a, b in zip(CB.ARRAYS, cat, bag):
                        assert np.array_equal(a, b), f"rows {rows} dim {dim} vocab {vocab}, {steps} step(s): {name} differs"


def test_recorded_digests():
    """Every recorded case recomputed with the library under test; where the padded and the CSR route both exist,
    cond_bits_cases.digests asserts that they give one digest."""
    with open(CB.GOLDEN) as f:
        want = json.load(f)["digests"]
    got = CB.digests()
    assert sorted(got) == sorted(want), "the recorded cases are not the cases of cond_bits_cases.digests()"
    wrong = [f"{case}: {array}" for case in sorted(want) for array in CB.ARRAYS if got[case][array] != want[case][array]]
    assert not wrong, "bits differ from tests/golden/cond_bits.json in " + "; ".join(wrong)
