"""The forward dispatch as data (dadmm_hip.ops.plan_forward): which launchers forward_raw tries,
in which order, and the sizes it allocates and zeroes. No GPU: the library's size queries run on
the host (the CU count falls back to 256 without a device)."""
import ctypes
import itertools

import pytest

from dadmm_hip import _lib
from dadmm_hip.ops import ForwardPlan, _split_cols, plan_forward

M, K = 64, 25
SERVES = (64, 5, 256)         # dadmm_split_scratch_bytes != 0
NOT_SERVED = (4096, 5, 256)   # fills more than half the CUs


def _dims(B, P, n, K=K):
    return _lib.Dims(B=B, P=P, m=M, n=n, K=K, variant=_lib.VARIANT_UNFOLDED, hyp_rows=1,
                     graph_shared=1)


def _serves(shape):
    return _lib.load().dadmm_split_scratch_bytes(ctypes.byref(_dims(*shape))) != 0


def test_the_library_serves_the_shapes_the_cases_assume():
    for shape in ((16, 5, 256), SERVES, (2048, 5, 256), (1024, 4, 128)):
        assert _serves(shape), shape
    for shape in ((2064, 5, 256), NOT_SERVED, (64, 5, 64), (64, 7, 256)):
        assert not _serves(shape), shape


def _expected(serves, fused_ok, path, record, train_split):
    """(candidates, gated) of the dispatch table, or ValueError."""
    tiled = "tiled_record" if record else "tiled"
    if path == "auto":
        if fused_ok and serves and (not record or train_split):
            return ("split",), True
        return (("fused", tiled) if fused_ok else (tiled,)), True
    if path == "fused":
        return (("fused",), False) if fused_ok else ValueError
    if path == "split":
        return (("split",), False) if fused_ok and serves else ValueError
    if path == "tiled":
        return (tiled,), False
    return (), True


# every row of the table, written out: (shape, fused_ok, path, record, train_split) -> plan
LITERAL = [
    (SERVES, True, "auto", False, False, ("split",), True),
    (SERVES, True, "auto", True, True, ("split",), True),
    (SERVES, True, "auto", True, False, ("fused", "tiled_record"), True),
    (NOT_SERVED, True, "auto", False, False, ("fused", "tiled"), True),
    (NOT_SERVED, True, "auto", True, True, ("fused", "tiled_record"), True),
    (SERVES, False, "auto", False, False, ("tiled",), True),
    (SERVES, False, "auto", True, True, ("tiled_record",), True),
    (NOT_SERVED, False, "auto", True, False, ("tiled_record",), True),
    (SERVES, True, "fused", False, False, ("fused",), False),
    (NOT_SERVED, True, "fused", True, True, ("fused",), False),
    (SERVES, True, "split", False, False, ("split",), False),
    (SERVES, True, "split", True, False, ("split",), False),
    (SERVES, True, "tiled", False, False, ("tiled",), False),
    (NOT_SERVED, False, "tiled", True, False, ("tiled_record",), False),
    (SERVES, True, "stepwise", False, False, (), True),
    (NOT_SERVED, False, "stepwise", True, True, (), True),
    # half the CUs: ceil(B / 16) <= 128 of the 256 CUs assumed without a device
    ((2048, 5, 256), True, "auto", False, False, ("split",), True),
    ((2064, 5, 256), True, "auto", False, False, ("fused", "tiled"), True),
    # the shape rule: P <= 6, n_pad 128 or 256
    ((64, 7, 256), True, "auto", False, False, ("fused", "tiled"), True),
    ((64, 7, 256), True, "auto", True, True, ("fused", "tiled_record"), True),
    ((64, 5, 64), True, "auto", False, False, ("fused", "tiled"), True),
    ((1024, 4, 128), True, "auto", False, False, ("split",), True),
]


@pytest.mark.parametrize("shape,fused_ok,path,record,train_split,candidates,gated", LITERAL)
def test_candidate_table_literal(shape, fused_ok, path, record, train_split, candidates, gated):
    plan = plan_forward(_dims(*shape), fused_ok, path=path, record=record, train_split=train_split)
    assert isinstance(plan, ForwardPlan)
    assert plan.candidates == candidates
    assert plan.gated is gated


ALL = list(itertools.product((SERVES, NOT_SERVED), (True, False),
                             ("auto", "fused", "split", "tiled", "stepwise"),
                             (False, True), (False, True)))


@pytest.mark.parametrize("shape,fused_ok,path,record,train_split", ALL)
def test_every_combination_and_its_sizes(shape, fused_ok, path, record, train_split):
    d = _dims(*shape)
    want = _expected(_serves(shape), fused_ok, path, record, train_split)
    kw = dict(path=path, record=record, train_split=train_split)
    if want is ValueError:
        with pytest.raises(ValueError):
            plan_forward(d, fused_ok, **kw)
        return
    plan = plan_forward(d, fused_ok, **kw)
    assert (plan.candidates, plan.gated) == want
    L, dp = _lib.load(), ctypes.byref(d)
    split = "split" in plan.candidates
    assert plan.split_bytes == (L.dadmm_split_scratch_bytes(dp) if split else 0)
    assert plan.split_flag_bytes == (L.dadmm_split_flag_bytes(dp) if split else 0)
    assert split == (plan.split_bytes != 0) == (plan.split_flag_bytes != 0)
    assert plan.stepwise_bytes == (L.dadmm_stepwise_scratch_bytes(dp) if plan.gated else 0)
    assert plan.gated == (plan.stepwise_bytes != 0)
    assert plan.nzero == (256 + plan.split_flag_bytes
                          + (4 * (8 + 4 * K) if plan.gated else 0)) // 4
    # split_cols decides through the same plan
    if path == "auto":
        assert _split_cols(d, fused_ok, record, train_split) == (64 if split else 0)


@pytest.mark.parametrize("shape", (SERVES, NOT_SERVED, (2048, 5, 256), (64, 7, 256)))
@pytest.mark.parametrize("fused_ok", (True, False))
@pytest.mark.parametrize("path", ("auto", "tiled", "stepwise"))
def test_train_split_without_record_changes_nothing(shape, fused_ok, path):
    d = _dims(*shape)
    assert plan_forward(d, fused_ok, path=path, train_split=True) == plan_forward(d, fused_ok,
                                                                                  path=path)


def test_plan_is_immutable():
    plan = plan_forward(_dims(*SERVES), True)
    with pytest.raises(AttributeError):
        plan.gated = False


def test_value_errors_keep_their_texts():
    d = _dims(*SERVES)
    with pytest.raises(ValueError, match="unknown path 'resident'"):
        plan_forward(d, True, path="resident")
    for path in ("fused", "split"):
        with pytest.raises(ValueError, match="follows non-ascending adjacency orders only for"):
            plan_forward(d, False, path=path)
    for record in (False, True):
        with pytest.raises(ValueError, match=r"the column-split forward does not serve "
                                             r"B=4096 P=5 n=256"):
            plan_forward(_dims(*NOT_SERVED), True, path="split", record=record)
