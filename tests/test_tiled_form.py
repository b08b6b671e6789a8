"""CPU: dadmm_tiled_form, the query that tells which form dadmm_forward_tiled /
dadmm_forward_tiled_record runs for a shape (1 the streamed single launch of csrc/dadmm_stream.hip,
0 the per-iteration launches of csrc/dadmm_tiled.hip, or the negative code the entry point returns
before launching). It asks the predicate the launch asks, so these cases pin the streamed form's
domain: P <= 16 at m <= 64, P <= 8 at 64 < m <= 128 (the reference's default shape P = 5, m = 100,
n = 500, configurations.py:6-9), at least four 32-column blocks. Nothing is launched."""
import pytest

UNSUPPORTED = -2


@pytest.fixture()
def form(monkeypatch):
    from dadmm_hip import _lib, tiled_form
    _lib.load()
    monkeypatch.delenv("DADMM_TILED_STREAM", raising=False)
    monkeypatch.delenv("DADMM_STREAM_WAVES", raising=False)
    return tiled_form


def test_the_binding_declares_the_query():
    from dadmm_hip import _lib
    assert _lib.ABI_VERSION >= 20
    assert "dadmm_tiled_form" in _lib.EXPORTED_SYMBOLS
    assert _lib.DADMM_EUNSUPPORTED == UNSUPPORTED


@pytest.mark.parametrize("shape", [(5, 100, 500), (8, 128, 128), (1, 65, 192), (16, 64, 512)])
def test_streamed_shapes(form, monkeypatch, shape):
    assert form(shape, record=True) == 1
    monkeypatch.setenv("DADMM_TILED_STREAM", "1")
    assert form(shape) == 1
    assert form(shape, record=True) == 1


def test_m64_streams_by_default(form):
    assert form((16, 64, 512)) == 1


def test_more_than_eight_agents_at_m128_take_the_launches(form, monkeypatch):
    monkeypatch.setenv("DADMM_TILED_STREAM", "1")
    assert form((9, 100, 500)) == 0
    assert form((9, 100, 500), record=True) == UNSUPPORTED


def test_stream_switched_off(form, monkeypatch):
    monkeypatch.setenv("DADMM_TILED_STREAM", "0")
    assert form((5, 100, 500)) == 0
    assert form((16, 64, 512)) == 0
    assert form((5, 100, 500), record=True) == 1   # recording has the streamed form only


def test_unsupported_shapes(form, monkeypatch):
    from dadmm_hip import _lib
    monkeypatch.setenv("DADMM_TILED_STREAM", "1")
    assert form((5, 129, 500)) == UNSUPPORTED
    assert "129" in _lib.load().dadmm_last_error().decode()
    assert form((5, 129, 500), record=True) == UNSUPPORTED
    assert form((5, 100, 64), record=True) == UNSUPPORTED   # n_pad = 64: two blocks, the ring needs four
    assert form((5, 100, 64)) == 0
    assert form((5, 100, 502)) == UNSUPPORTED                # n % 4


@pytest.mark.parametrize("shape", [(5, 100, 500), (8, 128, 128), (1, 65, 192)])
def test_sixteen_waves_never_run_two_m_groups(form, monkeypatch, shape):
    """DADMM_STREAM_WAVES=16 (one agent per wave, 128 VGPRs) has no m_pad = 128 build."""
    monkeypatch.setenv("DADMM_STREAM_WAVES", "16")
    monkeypatch.setenv("DADMM_TILED_STREAM", "1")
    assert form(shape) == 0
    assert form(shape, record=True) == UNSUPPORTED
    assert form((16, 64, 512)) == 1


def test_dims_struct_and_empty_work(form, monkeypatch):
    from dadmm_hip import _lib
    monkeypatch.setenv("DADMM_TILED_STREAM", "1")
    d = _lib.Dims(B=32, P=5, m=100, n=500, K=25, variant=0, hyp_rows=5, graph_shared=0)
    assert form(d) == 1 and form(d, record=True) == 1
    d.B = 0
    assert form(d) == 0
    d.B, d.hyp_rows = 32, 3
    assert form(d) == -1


def test_auto_records_small_batches_of_two_m_groups_on_the_stepwise_kernels(form):
    """plan_forward: at m > 64 the streamed recording launch is a candidate on 'auto' only from
    STREAM_RECORD_M128_MIN_B samples on (below it the stepwise recording is faster); path='tiled'
    takes it at every batch size, and m <= 64 is not affected."""
    from dadmm_hip import _lib, ops

    def plan(B, m, **kw):
        d = _lib.Dims(B=B, P=5, m=m, n=500, K=25, variant=0, hyp_rows=5, graph_shared=1)
        return ops.plan_forward(d, True, record=True, **kw).candidates
    big = ops.STREAM_RECORD_M128_MIN_B
    assert plan(32, 100) == ("fused",)
    assert plan(big - 1, 100) == ("fused",)
    assert plan(big, 100) == ("fused", "tiled_record")
    assert plan(32, 100, path="tiled") == ("tiled_record",)
    assert plan(32, 64) == ("fused", "tiled_record")
    d = _lib.Dims(B=32, P=5, m=100, n=500, K=25, variant=0, hyp_rows=5, graph_shared=1)
    assert ops.plan_forward(d, True).candidates == ("fused", "tiled")   # inference: unchanged
