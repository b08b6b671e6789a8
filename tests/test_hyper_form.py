"""CPU: dadmm_hyper_form, the query that tells which kernel form a hypernetwork launch takes (the
row tile WR of linear_kernel, the LDS-DMA operand ring, the K split over two wave sets, the split
input, the 32x32 inference kernel; for the stand-alone GCN block backward the workgroup size NT and
the register rows PR), or the negative code the launch would fail with. It asks launch_hyper's and
launch_gcn_bwd's own planning functions (plan_hyper, plan_gcn_bwd), so these cases pin the forms
that tests/test_gpu_hyper_train_kernels.py reaches, shape by shape, and what becomes of a sample of
129..160 nodes on a small grid: pick_tiles's fallback takes the 160-row tile (it used to return no
tile, and the launch failed with hipErrorInvalidValue), and the training epilogue, whose LDS holds
two tiles, one sample's A_hat and the column tables, stops at P = 137. Nothing is launched."""
import pytest

EINVAL, EUNSUPPORTED = -1, -2

# (B, P, K, N) -> (wr, dma, ks, samples per tile, grid): the tile forms of the GCN-class launches
# (the same for "gcn_train" and "linear_gcn_bwd"; ks: see KS2)
TILE_FORMS = {
    (12, 5, 64, 68): (1, 0, 1, 6, 4),          # two column tiles, the second 4 wide
    (640, 8, 64, 384): (2, 0, 1, 8, 480),      # only the 64-row candidate reaches 480 workgroups
    (3, 50, 64, 68): (2, 0, 1, 1, 6),          # P > 32 at a small grid: one sample per tile
    (1230, 7, 64, 448): (4, 0, 1, 18, 483),    # 18 x 7 = 126 of 128 rows: the best fill
    (2250, 5, 64, 448): (5, 0, 1, 32, 497),    # 71 row tiles, the last holds 10 samples
    (2250, 5, 512, 448): (5, 1, 1, 32, 497),   # K / 16 = 32: the DMA ring
    (12, 2, 64, 68): (1, 0, 1, 16, 2),
    (12, 64, 64, 68): (2, 0, 1, 1, 24),
}
# the K split: GCN_TRAIN from K = 256 under 480 tiles
KS2 = {"gcn_train": (12, 5, 256, 100)}


@pytest.fixture()
def form(monkeypatch):
    from dadmm_hip import _lib, hyper_form
    _lib.load()
    monkeypatch.delenv("DADMM_GCN32", raising=False)
    monkeypatch.delenv("DADMM_HYPER_KW", raising=False)
    return hyper_form


def _err():
    from dadmm_hip import _lib
    return _lib.load().dadmm_last_error().decode()


def test_the_binding_declares_the_query():
    from dadmm_hip import _lib
    assert _lib.ABI_VERSION >= 21
    assert "dadmm_hyper_form" in _lib.EXPORTED_SYMBOLS
    assert sorted(_lib.HYPER_FORM_KINDS.values()) == list(range(6))


@pytest.mark.parametrize("kind", ["gcn_train", "linear_gcn_bwd", "gcn"])
@pytest.mark.parametrize("shape", sorted(TILE_FORMS))
def test_tile_forms(form, kind, shape):
    wr, dma, ks, st, grid = TILE_FORMS[shape]
    f = form(kind, *shape)
    assert isinstance(f, dict), _err()
    assert (f["wr"], f["dma"], f["ks"], f["samples_per_tile"], f["grid"]) == (wr, dma, ks, st, grid)
    assert f["split"] == 0 and f["gcn32"] == 0 and f["nt"] == 0 and f["pr"] == 0


def test_k_split_over_two_wave_sets(form):
    for kind, shape in KS2.items():
        f = form(kind, *shape)
        assert (f["wr"], f["ks"], f["dma"], f["samples_per_tile"]) == (1, 2, 0, 6), (kind, f)
    # the C ABI's fused backward promises the bits of dadmm_hyper_linear + dadmm_hyper_gcn_train_bwd,
    # and dadmm_hyper_linear never splits: neither does it (the training backward's own fused launch,
    # which pairs with the GCN-class input-gradient GEMM, is not a C-ABI entry)
    assert form("linear_gcn_bwd", 12, 5, 128, 68)["ks"] == 1
    assert form("linear_gcn_bwd", 12, 5, 256, 100)["ks"] == 1
    assert form("gcn_train", 12, 5, 128, 100)["ks"] == 1      # the training forward splits from K = 256
    assert form("gcn", 12, 5, 256, 100)["ks"] == 1            # the inference layer never splits
    assert form("linear", 60, 1, 256, 100)["ks"] == 1         # nor do the C ABI's linears
    assert form("gcn_train", 12, 5, 512, 100)["ks"] == 1      # 32 k-steps: the ring's length, 32-row tiles
    assert form("gcn_train", 2250, 5, 256, 448)["ks"] == 1    # a full grid


def test_split_input(form):
    f = form("gcn_train", 12, 5, 128, 68, 64)
    assert (f["wr"], f["ks"], f["split"], f["dma"]) == (1, 1, 1, 0)
    assert form("gcn", 2250, 5, 512, 448, 256)["split"] == 1
    assert form("linear", 129, 1, 36, 65, 16)["split"] == 1
    assert form("gcn_train", 12, 5, 128, 68, 72) == EUNSUPPORTED      # K1 % 16
    assert "K1" in _err()
    assert form("linear_gcn_bwd", 12, 5, 128, 68, 64) == EINVAL       # one input only
    assert form("head", 12, 1, 128, 68, 64) == EINVAL


@pytest.mark.parametrize("shape,nt,pr,grid", [((12, 5, 68), 256, 8, 24), ((5, 9, 68), 256, 0, 10),
                                              ((2048, 2, 64), 64, 8, 2048), ((1024, 9, 128), 64, 0, 2048),
                                              ((12, 8, 68), 256, 8, 24), ((3, 64, 68), 256, 0, 6),
                                              ((2047, 2, 64), 256, 8, 2047)])
def test_gcn_backward_forms(form, shape, nt, pr, grid):
    B, P, N = shape
    f = form("gcn_bwd", B, P, 4, N)
    assert (f["nt"], f["pr"], f["grid"]) == (nt, pr, grid)
    assert f["wr"] == 0 and f["ks"] == 0


@pytest.mark.parametrize("B,H", [(64, 5), (7, 1), (300, 16)])
def test_head_forms(form, B, H):
    f = form("head", B, 1, 36, 4 * H)
    assert (f["wr"], f["dma"], f["ks"], f["split"]) == (1, 0, 1, 0)
    assert f["grid"] == (B + 31) // 32 * ((4 * H + 63) // 64)


def test_decoder_linear_forms(form):
    assert form("linear", 37, 1, 36, 100)["wr"] == 1
    assert form("linear", 2064, 1, 448, 224)["wr"] == 1        # 65 x 4 tiles: a small grid
    assert form("linear", 9000, 1, 1000, 400) == dict(wr=4, dma=1, ks=1, split=0, gcn32=0, nt=0, pr=0,
                                                      grid=71 * 7, samples_per_tile=0)


def test_inference_takes_the_32x32_kernel_on_full_grids(form):
    f = form("gcn", 1024, 50, 400, 400)
    assert f["gcn32"] == 1 and f["wr"] == 0 and f["samples_per_tile"] == 5
    assert form("gcn_train", 1024, 50, 400, 400)["gcn32"] == 0
    assert form("gcn", 3, 50, 400, 400)["gcn32"] == 0          # a small grid


@pytest.mark.parametrize("P", [129, 130, 137, 160])
def test_large_samples_on_a_small_grid_take_the_160_row_tile(form, P):
    """pick_tiles's fallback loop started at the 128-row tile, held no sample of 129..160 nodes and
    returned no tile; the launch then failed with hipErrorInvalidValue."""
    f = form("gcn", 3, P, 64, 68)
    assert isinstance(f, dict), _err()
    assert (f["wr"], f["samples_per_tile"], f["grid"], f["ks"], f["dma"]) == (5, 1, 6, 1, 0)
    assert form("gcn", 1, P, 512, 4)["wr"] == 5                # one workgroup; 32 k-steps: the ring
    assert form("gcn", 1, P, 512, 4)["dma"] == 1
    if P <= 137:
        f = form("gcn_train", 3, P, 64, 68)
        assert isinstance(f, dict), _err()
        assert (f["wr"], f["samples_per_tile"], f["grid"]) == (5, 1, 6)
        assert form("gcn_train", 480, P, 64, 68)["wr"] == 5    # and on a full grid, as before
    assert form("gcn", 480, P, 64, 68)["gcn32"] == 1           # (where inference takes the 32x32 kernel)


def test_p_limits(form):
    assert form("gcn", 3, 161, 64, 68) == EINVAL
    assert "P=161" in _err()
    assert form("gcn", 3, 0, 64, 68) == EINVAL
    # the training tile of one sample (two [160][68] tiles, A_hat [P][P], the column tables) fills
    # the 160 KB LDS at P = 137
    assert isinstance(form("gcn_train", 480, 137, 64, 68), dict)
    for B in (3, 480):
        assert form("gcn_train", B, 138, 64, 68) == EINVAL
        assert "P=138" in _err() and "137" in _err()
    assert form("gcn_train", 3, 1, 64, 68) == EINVAL           # BatchNorm over one node
    assert form("linear_gcn_bwd", 3, 65, 64, 68) == EINVAL
    assert form("gcn_bwd", 3, 65, 64, 68) == EINVAL
    assert "P=65" in _err()


def test_gcn_train_refuses_more_than_137_nodes_before_launching():
    """The entry point itself: DADMM_EINVAL and a message naming P, at every batch size (the launch
    used to fail with a HIP error: invalid value on small grids, invalid configuration on full ones)."""
    import ctypes

    from dadmm_hip import _lib
    L = _lib.load()
    fk = lambda i: ctypes.c_void_p(0x10000 * (i + 1))   # noqa: E731  16-B aligned, never touched
    for B in (3, 480):
        rc = L.dadmm_hyper_gcn_train(B, 138, 64, 68, fk(0), 64, 64, None, 0, fk(1), fk(2), fk(3), 1, fk(4),
                                     fk(5), 1e-5, 0.01, 0.1, 1, 0, fk(6), 68, fk(7), fk(8), fk(9), None, None,
                                     None)
        assert rc == EINVAL
        assert "P=138" in L.dadmm_last_error().decode()


def test_unknown_kind_bad_dims_and_empty_work(form):
    import ctypes

    from dadmm_hip import _lib
    L = _lib.load()
    f = _lib.HyperForm()
    assert L.dadmm_hyper_form(6, 12, 5, 64, 68, 64, ctypes.byref(f)) == EINVAL
    assert L.dadmm_hyper_form(3, 12, 5, 64, 68, 64, None) == EINVAL
    assert form("gcn_train", 12, 5, 66, 68) == EUNSUPPORTED    # K % 4
    assert form("gcn_train", 12, 5, 64, 66) == EUNSUPPORTED    # N % 4 (the float4 stores of M)
    assert form("gcn", 12, 5, 64, 66)["wr"] == 1               # the inference layer takes any N
    assert form("gcn_train", 12, 5, 0, 68) == EINVAL
    f = form("gcn_train", 0, 5, 64, 68)
    assert f["grid"] == 0 and f["wr"] == 0                     # nothing is launched
    assert _err() == ""
