"""The pending-r case of hmg_cell_histogram (option "lazy_r", tests/test_gpu_lazy_r.py): the call is handed r behind a lazy V-cycle,
settles the record exactly once through check_vec like hmg_cell_extrema, and its counts, r and x equal the eager run's bit for bit.

tests/test_gpu_lazy_r.py asks every ABI function with an hmg_vec argument for such a case in its READERS table
(test_every_vector_entry_has_a_case).  This module registers the case there when it is imported -- pytest imports every test module
of a run before the first test starts -- and runs it through that file's own test body, so the case is held to exactly what the
others are (the way of tests/test_gpu_lazy_r_cell_extrema_where.py)."""
import pytest

import homogenization_jl_amd as hmg
import test_gpu_lazy_r as LR
from test_gpu_lazy_r import ctx, problems      # noqa: F401  (that file's fixtures: its problems, its context)


@LR.reader("hmg_cell_histogram")
def cell_histogram(P, st):
    return (hmg.cell_histogram(st[-1].r, P.g, emin=-40, emax=24, sub_bits=4),)


def test_the_case_is_registered():
    assert LR.READERS["cell_histogram"][0] == ("hmg_cell_histogram",)
    LR.test_every_vector_entry_has_a_case()


@pytest.mark.gpu
def test_cell_histogram_sees_the_eager_r(ctx, problems):      # noqa: F811
    LR.test_every_reader_sees_the_eager_r(ctx, problems, "cell_histogram")
