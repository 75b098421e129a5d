"""CPU: the host side of ``spVIPES.transport_project`` -- its signature, every refusal ahead of any device work and of anything
written, the one-hot encoding of a label column and the frame a label projection comes back as.  No GPU."""
import inspect

import numpy as np
import pytest
import torch

from tests._duck import make_duck


class _Plan:
    """stands for a TransportPlan where only its shape and the presence of potentials are looked at"""
    def __init__(self, shape):
        self.shape, self.sinkhorn = shape, object()


def _adata():
    ad = make_duck(n=(30, 20), G=(8, 8), seed=2)
    rng = np.random.default_rng(0)
    ad.obsm = {"X_rep": rng.standard_normal((50, 5)).astype(np.float32), "coords": rng.standard_normal((50, 3))}
    return ad


def test_signature():
    from spvipes_amd.model import spVIPES
    from spvipes_amd import ot_ops
    sig = inspect.signature(spVIPES.transport_project)
    assert list(sig.parameters) == ["adata", "use_rep", "plan", "values", "onto", "key_added", "device"]
    assert sig.parameters["onto"].default == 0 and sig.parameters["key_added"].default is None and sig.parameters["device"].default is None
    assert isinstance(inspect.getattr_static(spVIPES, "transport_project"), classmethod)
    assert list(inspect.signature(ot_ops.ot_project).parameters) == ["X", "Y", "h", "V", "inv_eps", "n_split", "out", "return_lse"]
    assert list(inspect.signature(ot_ops.transport_project).parameters) == ["res", "X_q", "X_c", "V", "side"]
    assert ot_ops.OT_VAL_MAX == 256


REFUSALS = [
    ("matrix-plan", dict(plan=np.zeros((30, 20), np.float32)), TypeError, r"plan\.to_scipy\(\) @ values"),
    ("plan-shape", dict(plan=_Plan((20, 30))), ValueError, "plan couples"),
    ("onto-2", dict(onto=2), ValueError, "onto must be 0 or 1"),
    ("onto-true", dict(onto=True), ValueError, "onto must be 0 or 1"),
    ("onto-str", dict(onto="a"), ValueError, "onto must be 0 or 1"),
    ("rows-of-the-receiving-group", dict(values=np.zeros((30, 2))), ValueError, r"one row per cell of group 1 \(20\)"),
    ("rows-wrong", dict(values=np.zeros((7, 2))), ValueError, "one row per cell"),
    ("rows-onto-1", dict(values=np.zeros((20, 2)), onto=1), ValueError, r"one row per cell of group 0 \(30\)"),
    ("values-1d", dict(values=np.zeros(20)), ValueError, "numeric array"),
    ("values-no-columns", dict(values=np.zeros((20, 0))), ValueError, "numeric array"),
    ("values-strings", dict(values=np.full((20, 2), "x")), ValueError, "numeric array"),
    ("values-nan", dict(values=np.where(np.arange(40).reshape(20, 2) == 7, np.nan, 1.0)), ValueError, "non-finite"),
    ("values-inf-in-the-other-group-only", dict(values=np.where(np.arange(100).reshape(50, 2) == 61, np.inf, 1.0)), ValueError, "non-finite"),
    ("values-beyond-fp32", dict(values=np.full((20, 2), 1e39)), ValueError, "non-finite"),
    ("unknown-key", dict(values="nope"), KeyError, "neither a key of adata.obsm nor a column of adata.obs"),
    ("unknown-use_rep", dict(use_rep="nope"), KeyError, "use_rep 'nope' not found"),
    ("use_rep-rows", dict(use_rep=np.zeros((49, 5), np.float32)), ValueError, "one row per cell"),
    ("use_rep-too-wide", dict(use_rep=np.zeros((50, 65), np.float32)), ValueError, "between 1 and 64 columns"),
    ("key_added-not-a-string", dict(key_added=3), ValueError, "key_added must be a string"),
]


@pytest.mark.parametrize("case,over,exc,text", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_come_before_any_device_work_and_write_nothing(case, over, exc, text, monkeypatch):
    from spvipes_amd.model import spVIPES
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for ahead of the refusal"))
    ad = _adata()
    kw = dict(dict(use_rep="X_rep", plan=_Plan((30, 20)), values="coords", onto=0, key_added="proj"), **over)
    with pytest.raises(exc, match=text):
        spVIPES.transport_project(ad, **kw)
    assert set(ad.obsm) == {"X_rep", "coords"} and "proj" not in ad.obs


def test_values_in_the_other_group_need_not_be_finite_in_the_receiving_one():
    """rows of the receiving group are never read: the checks pass and the call gets as far as asking for the device"""
    from spvipes_amd import _abi
    from spvipes_amd.model import spVIPES
    ad = _adata()
    vals = np.ones((50, 2))
    vals[:30] = np.nan   # group 0 receives
    if not torch.cuda.is_available():
        with pytest.raises(_abi.SpvError, match="MI355X"):
            spVIPES.transport_project(ad, "X_rep", _Plan((30, 20)), vals, onto=0)


def test_check_returns_the_other_groups_rows_and_one_hot_labels():
    from spvipes_amd.data import check_transport_project_args
    ad = _adata()
    rep = ad.obsm["X_rep"]
    obs_idx, X0, X1, V, cats = check_transport_project_args(ad, rep, _Plan((30, 20)), "coords", 0, None)
    assert cats is None and V.dtype == np.float32 and V.flags.c_contiguous
    np.testing.assert_array_equal(V, ad.obsm["coords"][30:].astype(np.float32))
    np.testing.assert_array_equal(X0, rep[:30]), np.testing.assert_array_equal(X1, rep[30:])
    _, _, _, V1, _ = check_transport_project_args(ad, rep, _Plan((30, 20)), ad.obsm["coords"][:30], 1, None)
    np.testing.assert_array_equal(V1, ad.obsm["coords"][:30].astype(np.float32))
    _, _, _, H, cats = check_transport_project_args(ad, rep, _Plan((30, 20)), "cell_type", 0, None)
    col = ad.obs["cell_type"][30:]
    np.testing.assert_array_equal(cats, np.unique(col))            # the categories among the OTHER group's cells only
    assert H.shape == (20, len(cats)) and H.dtype == np.float32 and (H.sum(1) == 1).all() and set(np.unique(H)) == {0.0, 1.0}
    np.testing.assert_array_equal(cats[H.argmax(1)], col)


def test_one_hot_and_frame_on_a_made_up_projection():
    from spvipes_amd.data import label_projection_frame, one_hot_labels
    cats, hot = one_hot_labels(np.array(["b", "a", "c", "a"]))
    assert list(cats) == ["a", "b", "c"]
    np.testing.assert_array_equal(hot, np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1], [1, 0, 0]], np.float32))
    probs = np.array([[0.2, 0.7, 0.1], [0.4, 0.4, 0.2], [0.0, 0.5, 0.5], [np.nan, np.nan, np.nan]], np.float32)
    frame = label_projection_frame(probs, cats, ["w", "x", "y", "z"])
    assert list(frame.columns) == ["a", "b", "c", "predicted", "confidence"] and list(frame.index) == ["w", "x", "y", "z"]
    assert list(frame["predicted"][:3]) == ["b", "a", "b"], "ties go to the first category"
    assert frame["predicted"].iloc[3] is None and np.isnan(frame["confidence"].iloc[3])
    np.testing.assert_array_equal(frame["confidence"].to_numpy()[:3], np.array([0.7, 0.4, 0.5], np.float32))
    np.testing.assert_array_equal(frame[["a", "b", "c"]].to_numpy()[:3], probs[:3])
    ints = label_projection_frame(probs[:3], np.array([3, 5, 9]), np.arange(3))
    assert list(ints.columns[:3]) == ["3", "5", "9"] and list(ints["predicted"]) == [5, 3, 5]
    with pytest.raises(ValueError):
        label_projection_frame(probs, cats[:2], ["w", "x", "y", "z"])
