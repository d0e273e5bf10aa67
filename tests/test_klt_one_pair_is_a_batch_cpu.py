"""No GPU: the rows of tests/test_klt_one_pair_is_a_batch_gpu.py cannot pass on empty or trivially full output.  The CPU restatements
(tests/indep_klt*.py) alone give every 128 x 96 row some kept tracks and some that are not, at least one status 5 where the forward-backward
check is on and at least one status 6 where the intra test is; the counts are pinned here, the GPU test asserts the same bounds on what the
device returned."""
import pytest

import klt_one_pair_cases as oc


@pytest.mark.parametrize("name,cell", oc.ROWS)
def test_the_restatement_keeps_some_tracks_and_drops_some(name, cell):
    slots = (oc.W // cell) * (oc.H // cell)
    for predicted in (False, True):
        ans = oc.expect(name, cell, predicted)
        assert len(ans["slots"]) == slots
        tally = oc.tally(ans["slots"])
        assert tally == oc.PINNED[(name, cell)][predicted], (name, cell, predicted, tally)
        assert tally[0] == ans["count"]
        assert oc.bounds_hold(name, cell, tally, slots), (name, cell, predicted, tally)


def test_the_rows_cover_the_issue_and_the_pair_is_not_cut():
    assert set(oc.SETTINGS) == {"plain", "n3m", "n3f", "n3m_n3f", "intra_cut", "n3f_intra"} and oc.CELLS == (8, 16)
    assert oc.PADDED_ROW in oc.ROWS and oc.NO_SLOTS_ROW in oc.ROWS
    for cell in oc.CELLS:
        for predicted in (False, True):
            assert not oc.expect("intra_cut", cell, predicted)["cut"]
    big = oc.LARGE
    assert ((big["W"] + 7) // 8) * ((big["H"] + 7) // 8) == big["slots"] > 32768 and big["kept_above"] == 16384
