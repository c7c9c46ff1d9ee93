"""The pending-r case of hmg_cell_histogram_groups (option "lazy_r", tests/test_gpu_lazy_r.py): the call is handed r behind a lazy
V-cycle, settles the record exactly once through check_vec -- it runs the pass of hmg_cell_histogram --, and its group counts and
volumes, r and x equal the eager run's bit for bit.

tests/test_gpu_lazy_r.py asks every ABI function with an hmg_vec argument for such a case in its READERS table
(test_every_vector_entry_has_a_case).  This module registers the case there when it is imported -- pytest imports every test module
of a run before the first test starts -- and runs it through that file's own test body, so the case is held to exactly what the
others are (the way of tests/test_gpu_lazy_r_cell_histogram.py)."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
import test_gpu_lazy_r as LR
from test_gpu_lazy_r import ctx, problems      # noqa: F401  (that file's fixtures: its problems, its context)


@LR.reader("hmg_cell_histogram_groups")
def cell_histogram_groups(P, st):
    ne = P.g.ncells()
    labels = (np.arange(ne) * 5) % 3 - (np.arange(ne) % 7 == 0)        # three groups, unsorted; every seventh cell may fall out (-1)
    weights = 1.0 / (1.0 + np.arange(ne))
    _, counts, volume = hmg.cell_histogram_groups(st[-1].r, P.g, labels, weights=weights, emin=-40, emax=24, sub_bits=4)
    return counts, volume


def test_the_case_is_registered():
    assert LR.READERS["cell_histogram_groups"][0] == ("hmg_cell_histogram_groups",)
    LR.test_every_vector_entry_has_a_case()


@pytest.mark.gpu
def test_cell_histogram_groups_sees_the_eager_r(ctx, problems):      # noqa: F811
    LR.test_every_reader_sees_the_eager_r(ctx, problems, "cell_histogram_groups")
