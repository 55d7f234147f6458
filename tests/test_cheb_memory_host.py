"""Host side of the Chebyshev family's memory-contract tests: the case table of tests/cheb_memory_ref.py has finite float64
references of the sizes it states, its references equal the oracle's own functions, and the wrappers' decision to hand the
fused kernels an aligned copy (``_native._aligned16`` / ``_native._fused_x``: pure Python) is right on CPU tensors."""

import numpy as np
import pytest
import torch

import cheb_memory_ref as R
from deepsphere import _native
from oracle import cheb_oracle as orc


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_reference_is_finite_and_has_the_tables_sizes(name):
    d = R.data(name)
    case, g = d["case"], d["graph"]
    rows, W = g["cols"].shape
    assert g["vals"].shape == (rows, W) and g["vals"].dtype == np.float32 and g["cols"].dtype == np.int32
    assert 0 <= g["cols"].min() and g["cols"].max() < g["n_cols"]
    assert d["x"].shape == (case.N, g["n_cols"], case.Fin) and d["x"].dtype == np.float32
    assert d["ref"].dtype == np.float64 and d["ref"].shape == R.out_shape(case, g)
    assert np.all(np.isfinite(d["ref"])) and np.abs(d["ref"]).max() > 0.1
    if case.kind == "planes":
        assert d["w"] is None and d["ref"].shape == (case.K - 1, case.N, rows, case.Fin)
    elif case.kind == "wgrad":
        assert d["dy"].shape == (case.N, rows, case.Fout) and d["ref"].shape == (case.Fin * case.K, case.Fout)
        assert d["planes"].shape == (case.K, case.N, rows, case.Fin)
    else:
        assert d["w"].shape == (case.Fin * case.K, case.Fout) and (d["bias"] is not None) == case.bias
        out_rows = rows // 4 if case.kind == "pool" else g["out_rows"]
        assert d["ref"].shape == (case.N, out_rows, case.Fout)
    if case.graph[0] == "grid_drop":
        assert rows % 256 != 0, "the last tile of this map is incomplete"
    if case.kind == "parts":
        assert g["n_cols"] > g["out_rows"] and len(g["levels"]) == case.K - 1 and g["out_rows"] % 256 == 0
    assert R.tolerance(case) in (2e-6, 1e-5, 2e-5, 1e-5 * 5, 2e-6 * 5)
    assert R.data(name) is d, "one reference per case: the variants share it"


def test_table_covers_the_routes_of_the_audit():
    kinds = {c.kind for c in R.CASES}
    assert kinds == {"forward", "pool", "planes", "wgrad", "parts"}
    assert {c.route for c in R.CASES} == {"unfused", "bfs", "struct", "strips", "chain"}
    assert {c.prec for c in R.CASES if c.route in ("bfs", "unfused")} >= {"fp32", "bf16x3"}
    assert all(c.y_off in ("same", "tiles", "close") and c.bias_off in ("same", "tiles") for c in R.CASES)
    assert all(c.bias_off == "tiles" for c in R.CASES if c.name.startswith(("quad_", "q8_")))


@pytest.mark.parametrize("name", ["unfused_8_12_4", "tiled_wide_4_12_3", "bfs_16_32_5_fp32", "pool_4_8_5", "wgrad_bfs_16_24_3"])
def test_references_equal_the_oracles_own_functions(name):
    d = R.data(name)
    case, g = d["case"], d["graph"]
    if case.kind == "wgrad":
        _, dW = orc.chebyshev_backward(g["Lt"], d["x"], np.zeros((case.Fin * case.K, case.Fout), np.float32), case.K, d["dy"])
        assert np.abs(dW - d["ref"]).max() <= 1e-10 * np.abs(dW).max()
        return
    fwd = orc.chebyshev_forward if case.basis == "chebyshev" else orc.monomial_forward
    y = fwd(g["Lt"], d["x"], d["w"], case.K, bias=d["bias"], activation=case.act)
    if case.kind == "pool":
        y = orc.healpy_pool(y, 1, "MAX")
    assert np.abs(y - d["ref"]).max() <= 1e-12 * np.abs(y).max()


def _off(n, offset):
    buf = torch.arange(n + offset, dtype=torch.float32)
    return buf[offset:]


def test_aligned16_copies_only_what_is_off_alignment():
    a = _off(64, 0)
    assert a.data_ptr() % 16 == 0 and _native._aligned16(a) is a
    for offset in (1, 2, 3):
        v = _off(64, offset).view(4, 16)
        assert v.data_ptr() % 16 == 4 * offset
        c = _native._aligned16(v)
        assert c is not v and c.data_ptr() % 16 == 0 and c.is_contiguous() and c.shape == v.shape and torch.equal(c, v)
    v4 = _off(64, 4)  # (16 bytes into a buffer is aligned)
    assert _native._aligned16(v4) is v4


class _Plan:
    """Stands in for a LaplacianPlan: records whether the wrapper asked it about the fused route."""

    def __init__(self, fused):
        self.fused, self.asked = fused, 0

    def fused_ok(self, Fin, Fout, K):
        self.asked += 1
        return self.fused


def test_fused_x_copies_only_on_the_fused_route():
    x, v = _off(2 * 8 * 16, 0).view(2, 8, 16), _off(2 * 8 * 16, 1).view(2, 8, 16)
    fused, plain = _Plan(True), _Plan(False)
    assert _native._fused_x(fused, x, 16, 32, 5, _native.ALGO_AUTO) is x and fused.asked == 0, "an aligned x costs no question"
    c = _native._fused_x(fused, v, 16, 32, 5, _native.ALGO_AUTO)
    assert c is not v and c.data_ptr() % 16 == 0 and torch.equal(c, v)
    assert _native._fused_x(fused, v, 16, 32, 5, _native.ALGO_FUSED) is not v
    assert _native._fused_x(fused, v, 16, 32, 5, _native.ALGO_UNFUSED) is v, "the unfused kernels have scalar forms"
    assert _native._fused_x(plain, v, 16, 32, 5, _native.ALGO_AUTO) is v and plain.asked == 1, "AUTO on a plan without fused kernels"
    v7 = _off(2 * 8 * 7, 1).view(2, 8, 7)
    assert _native._fused_x(fused, v7, 7, 32, 5, _native.ALGO_AUTO) is v7, "Fin % 4 != 0: the kernels read a padded copy in the workspace"
