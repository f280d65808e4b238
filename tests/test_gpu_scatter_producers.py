"""GPU (run with `-m gpu`): the two instantiations of the owner-binned hash-gradient scatter's producer kernel leave the same
gradient table.

f2n_set_scatter_producer(0) is the non-staged instantiation (hash constants from global memory, four blocks per CU); the default,
the staged instantiation, keeps its level's hash constants in dynamic LDS when they fit (the non-staged one otherwise), so three
blocks share a CU and take their slots in another order.  Which
slot of a queue segment a record lands in differs between them; what the owners make of a segment does not: they sum its records
exactly (fixed-point image or fp64).  So as long as no record takes the packed-f16 atomic of last resort
(f2n_debug_counters()[0] == 0) the two f16 tables are equal byte for byte -- the criterion here is equality, there is no tolerance.
(The run-structure extremes were chosen for a difference that was measured and not kept -- records compacted across the eight
corners through a wave-private staging area; they stay as inputs that fill, and that barely touch, every tile's record stores.)

Every case scatters ONE input with variant 0 and with the default into zeroed tables.  The binned path needs n >= 32768: the
smallest shape at which the kernel exists.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pipeline as op  # noqa: E402
import test_gpu_parity as gp  # noqa: E402  (gp.T / gp.N / gp.DEV through the module: the emulated run replaces them)
from test_gpu_parity import F32, make_grid, grid_dev, rand_params  # noqa: E402
from oracle import capi as oc  # noqa: E402

NEW = 1  # f2n_set_scatter_producer's default


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import capi
    capi.lib()
    return capi


def both_producers(hip, run):
    """run() -> tensors, once per producer; returns [(tensors, counters)] for variant 0 and the default."""
    out = []
    try:
        for variant in (0, NEW):
            hip.set_scatter_producer(variant)
            hip.debug_counters(reset=True)
            got = run()
            out.append((got, hip.debug_counters()))
    finally:
        hip.set_scatter_producer(NEW)
    return out


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------- inputs
def rays50(rng, n, n_volumes):
    """test_hash_backward_owner_binned's input: rays of 50 closely spaced samples, one transform per ray."""
    n_rays = n // 50 + 1
    o = rng.random((n_rays, 3), dtype=F32) * F32(.6) + F32(.2)
    dvec = rng.standard_normal((n_rays, 3)).astype(F32)
    dvec /= np.linalg.norm(dvec, axis=1, keepdims=True)
    ray = np.repeat(np.arange(n_rays), 50)[:n]
    step = (np.arange(n) % 50).astype(F32) * F32(0.004)
    q = np.clip(o[ray] + dvec[ray] * step[:, None], 0.01, 0.99).astype(F32)
    vol = rng.integers(0, n_volumes, n_rays).astype(np.int32)[ray]
    return q, vol


def one_cell_rows(rng, n, n_volumes):
    """Every row of 16 samples is one point in one transform: one run per row at every level, one record-owning lane per row."""
    rows = (n + 15) // 16
    q = np.repeat(rng.random((rows, 3), dtype=F32) * F32(.98) + F32(.01), 16, axis=0)[:n]
    vol = np.repeat(rng.integers(0, n_volumes, rows).astype(np.int32), 16)[:n]
    return np.ascontiguousarray(q), np.ascontiguousarray(vol)


def no_neighbours(rng, n, n_volumes):
    """Neighbouring samples in different transforms (the transform index is part of a cell's identity): no run longer than one
    sample at any level, every lane ends a run."""
    q = rng.random((n, 3), dtype=F32) * F32(.98) + F32(.01)
    vol = (np.arange(n) % min(4, n_volumes)).astype(np.int32)
    return q, vol


STRUCTURES = {"rays50": rays50, "one_cell_rows": one_cell_rows, "no_neighbours": no_neighbours}


def gradients(rng, n, kind):
    if kind == "dense":  # no zero gradient, and large enough that (almost) no corner's product rounds to zero: eight records per lane
        g = (rng.uniform(0.5, 1.0, (n, 32)) * rng.choice([-1.0, 1.0], (n, 32))).astype(np.float16)
    else:
        g = (rng.standard_normal((n, 32)) * 0.05).astype(np.float16)
    if kind == "half":  # the existing test's: half the samples zero
        g[rng.random(n) < 0.5] = 0
    elif kind == "zero":
        g[:] = 0
    elif kind == "one":
        keep = g[n // 3].copy()
        g[:] = 0
        g[n // 3] = keep
    elif kind == "half_rows":  # every other 16-sample row zero
        g[(np.arange(n) // 16) % 2 == 0] = 0
    return g


def scatter_case(hip, grid, q, vol, gin, log2):
    gd = grid_dev(grid)
    n = len(q)
    args = (n, grid.n_volumes, gd["prim"], gd["lidx"], gd["lsize"], gd["bias"], gd["scale"], gp.T(q), False, gp.T(vol), 1, gp.T(gin))

    def run():
        tab = torch.zeros(grid.table_f32.size, dtype=torch.float16, device=gp.DEV)
        hip.hash_bwd(*args, tab, 1 << log2)
        return tab
    (t0, c0), (t1, c1) = both_producers(hip, run)
    assert c0[0] == 0 and c1[0] == 0, (c0, c1)
    assert same_bytes(t0, t1), "%d of %d table halves differ" % (int((t0.view(torch.int16) != t1.view(torch.int16)).sum()), t0.numel())
    return t0, c0, c1


# ------------------------------------------------------------------------------------------------- f2n_hash_bwd
@pytest.mark.parametrize("structure", list(STRUCTURES))
@pytest.mark.parametrize("n", [32768, 32769, 40037])  # 32 chunks of exactly 1024; one sample more; ragged last chunk and last tile
def test_producers_agree_on_sizes_and_run_structures(hip, fox_state, n, structure):
    rng = np.random.default_rng(n + len(structure))
    grid = make_grid(fox_state, rng, 14, zeros=True)
    q, vol = STRUCTURES[structure](rng, n, grid.n_volumes)
    gin = gradients(rng, n, "dense" if structure == "no_neighbours" else "half")
    tab, _, _ = scatter_case(hip, grid, q, vol, gin, 14)
    assert bool((tab != 0).any())


@pytest.mark.parametrize("kind", ["zero", "one", "half_rows"])
def test_producers_agree_on_sparse_gradients(hip, fox_state, kind):
    rng = np.random.default_rng(5)
    n = 40037
    grid = make_grid(fox_state, rng, 14, zeros=True)
    q, vol = rays50(rng, n, grid.n_volumes)
    tab, _, _ = scatter_case(hip, grid, q, vol, gradients(rng, n, kind), 14)
    nz = int((tab != 0).sum())
    if kind == "zero":
        assert nz == 0  # no record at all
    elif kind == "one":
        assert 0 < nz <= 16 * 8 * 2  # one sample: at most eight entries per level
    else:
        assert nz > 0


@pytest.mark.parametrize("log2", [19, 20])  # (2^14: above) 2^19 the benched table, 2^20 the instantiation with overflow lists
def test_producers_agree_on_large_tables(hip, fox_state, log2):
    rng = np.random.default_rng(log2)
    n = 40037
    grid = make_grid(fox_state, rng, log2, zeros=True)
    q, vol = rays50(rng, n, grid.n_volumes)
    tab, _, _ = scatter_case(hip, grid, q, vol, gradients(rng, n, "half"), log2)
    assert bool((tab != 0).any())


def test_producers_agree_when_segments_overflow(hip, fox_state):
    """test_hash_backward_overflow_lists_keep_the_sums_order_free's tiny cube at 2^20 entries per level: as many records travel through
    the overflow lists with either producer (a segment takes the first `cap` records that ask, whoever they are)."""
    rng = np.random.default_rng(77)
    log2 = 20
    grid = make_grid(fox_state, rng, log2, zeros=True)
    n = 32768 + 1024 + 5
    q = (F32(0.371) + rng.random((n, 3), dtype=F32) * F32(2e-4)).astype(F32)
    vol = (np.arange(n) % 4).astype(np.int32)
    gin = (rng.standard_normal((n, 32)) * 0.01).astype(np.float16)
    _, c0, c1 = scatter_case(hip, grid, q, vol, gin, log2)
    assert c0[3] == c1[3] and c0[3] > 0, (c0, c1)


def test_producers_agree_with_more_transforms_than_the_lds_budget_holds(hip, fox_state):
    """A synthetic pool of 600 transforms: 24 B each, more than the 12288 B a producer block stages per level -- the launch falls back
    to global loads of the hash constants (the non-staged instantiation) whatever the setter says."""
    rng = np.random.default_rng(600)
    V, log2, n = 600, 14, 32769
    prim = (rng.integers(1, 1 << 30, (16, V, 3)) * 2 + 1).astype(np.int32)
    bias = rng.random((16 * V, 3), dtype=F32)
    grid = op.HashGrid(np.zeros((16 << log2, 2), F32), prim, bias, V, log2)
    q, vol = rays50(rng, n, V)
    tab, _, _ = scatter_case(hip, grid, q, vol, gradients(rng, n, "half"), log2)
    assert bool((tab != 0).any())


# ------------------------------------------------------------------------------------------------- f2n_field_bwd_dyn
N_OFF = 6
BIG = 135000  # a capacity the host sizes 64 chunks for; 40000 rows on the device make it 32


@pytest.mark.parametrize("cap,count", [(32768 + 5, 32768 + 5), (BIG, BIG - 1), (BIG, BIG), (BIG, 40000)])
def test_producers_agree_behind_the_field_backward(hip, fox_state, fox_golden, cap, count):
    """Planes layout, non-zero mask words and a device-side row count with a non-zero offset, the way a streaming step calls the
    scatter: weight gradients and gradient table of the two producers, bit for bit."""
    g = fox_golden
    rng = np.random.default_rng(cap + count)
    log2 = 14
    grid = make_grid(fox_state, rng, log2, scale=0.5)
    gd = grid_dev(grid)
    phf = gp.T(oc.f2h(rand_params(rng, 1)).view(np.float16))
    pick = rng.integers(0, len(g["march_pts"]), cap)
    pts, vol = gp.T(g["march_pts"][pick]), gp.T(np.ascontiguousarray(g["march_anchors"][pick, 0]))
    x = gp.T((rng.standard_normal((cap, 32)) * 0.5).astype(np.float16))
    dfeat = gp.T((rng.standard_normal((cap, 16)) * 1e-3).astype(F32))
    n_dev = torch.tensor([count - N_OFF], dtype=torch.int32, device=gp.DEV)

    def run():
        dW = torch.zeros(3072, device=gp.DEV)
        tab = torch.zeros(grid.table_f32.size, dtype=torch.float16, device=gp.DEV)
        hip.deferred_reset()
        hip.field_bwd_dyn(cap, n_dev, N_OFF, grid.n_volumes, gd["prim"], gd["lidx"], gd["lsize"], gd["bias"], gd["scale"], pts, vol, 1, phf,
                          x, dfeat, 128.0, dW, tab, 1 << log2, 1)
        hip.reduce_deferred()
        return dW, tab
    ((dw0, t0), c0), ((dw1, t1), c1) = both_producers(hip, run)
    assert c0[0] == 0 and c1[0] == 0, (c0, c1)
    assert bool((t0 != 0).any()) and float(dw0.abs().max()) > 0
    assert torch.equal(dw0.view(torch.int32), dw1.view(torch.int32))
    assert same_bytes(t0, t1)
