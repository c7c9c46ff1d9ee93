"""The pending-r case of hmg_cell_extrema_where (option "lazy_r", tests/test_gpu_lazy_r.py): the call is handed r behind a lazy
V-cycle, settles the record exactly once through check_vec like hmg_cell_extrema, and its five results, r and x equal the eager
run's bit for bit.

tests/test_gpu_lazy_r.py asks every ABI function with an hmg_vec argument for such a case in its READERS table
(test_every_vector_entry_has_a_case).  This module registers the case there when it is imported -- pytest imports every test module
of a run before the first test starts -- and runs it through that file's own test body, so the case is held to exactly what the
others are."""
import pytest

import homogenization_jl_amd as hmg
import test_gpu_lazy_r as LR
from test_gpu_lazy_r import ctx, problems      # noqa: F401  (that file's fixtures: its problems, its context)


@LR.reader("hmg_cell_extrema_where")
def cell_extrema_where(P, st):
    return hmg.cell_extrema_where(st[-1].r, P.g)


def test_the_case_is_registered():
    assert LR.READERS["cell_extrema_where"][0] == ("hmg_cell_extrema_where",)
    LR.test_every_vector_entry_has_a_case()


@pytest.mark.gpu
def test_cell_extrema_where_sees_the_eager_r(ctx, problems):      # noqa: F811
    LR.test_every_reader_sees_the_eager_r(ctx, problems, "cell_extrema_where")
