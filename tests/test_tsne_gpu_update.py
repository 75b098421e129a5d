"""GPU: spv_tsne_update (spvipes_amd.tsne_ops.update) against ``update_ref`` of tests/_tsne_reference.py on its ``update_case``: 300 rows, a
random symmetric CSR matrix with an empty row (5) and a full row (9), a previous step and gains of both kinds, float64 Zrow / F from the
reference.  ``update_ref``'s docstring derives the bounds: (D + 7) 2^-24 of the attractive terms' magnitudes on the gradient, (D + 4)
2^-24 of the row's mass on kl_row, the step's own fp32 roundings on u and y_out, fp64 terms throughout.  A gain may differ from the
reference's only where the reference's |g| is below its own error bound (the sign test is open there), on at most 1 % of the elements
(tests/test_tsne_reference_cpu.py holds the reference alone to that); everywhere else it is the reference's bit for bit.  Every test
here imports the new function and fails without it."""
import numpy as np
import pytest
import torch

from tests import _tsne_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _call(dev, c, with_outputs=True):
    from spvipes_amd.tsne_ops import update
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("indptr", "cols", "vals", "y", "u", "gain", "Zrow", "F")}
    n, D = c["n"], c["D"]
    y_out = torch.full((n, D), float("nan"), dtype=torch.float32, device=dev)
    Z = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    kl = torch.full((n,), float("nan"), dtype=torch.float64, device=dev) if with_outputs else None
    grad = torch.full((D, n), float("nan"), dtype=torch.float64, device=dev) if with_outputs else None
    update(t["y"], y_out, t["indptr"], t["cols"], t["vals"], t["Zrow"], t["F"], Z, t["u"], t["gain"], c["alpha"], c["momentum"], c["lr"], c["min_gain"],
           kl_row=kl, grad=grad)
    torch.cuda.synchronize()
    assert torch.equal(t["y"].cpu(), torch.from_numpy(c["y"])), "y_in is only read"
    return {"y_out": y_out.cpu().numpy(), "Z": float(Z.cpu()[0]), "u": t["u"].cpu().numpy(), "gain": t["gain"].cpu().numpy(),
            "kl_row": None if kl is None else kl.cpu().numpy(), "grad": None if grad is None else grad.cpu().numpy()}


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_update_against_the_reference(dev, D):
    c = R.update_case(D=D)
    r = R.update_ref(c)
    got = _call(dev, c)
    n = c["n"]
    assert abs(got["Z"] - r["Z"]) <= (n + 8) * 2.0 ** -53 * r["Z"]
    eg = np.abs(got["grad"] - r["grad"])
    assert (eg <= r["e_grad"]).all(), f"gradient: worst {np.max(eg / r['e_grad']):.3g} of its bound"
    ek = np.abs(got["kl_row"] - r["kl_row"])
    assert (ek <= r["e_kl"]).all() and got["kl_row"][5] == 0.0, f"kl_row: worst {np.max(ek / np.maximum(r['e_kl'], 1e-300)):.3g} of its bound"
    open_ = r["unsure"]
    assert open_.mean() <= 0.01
    differs = got["gain"] != r["gain"]
    assert not (differs & ~open_).any(), "a gain differs where the reference is sure of the sign"
    assert (got["gain"] >= np.float32(c["min_gain"])).all()
    same = ~differs
    assert (np.abs(got["u"] - r["u"])[same] <= r["e_u"][same]).all() and (np.abs(got["y_out"] - r["y_out"])[same] <= r["e_y"][same]).all()
    assert np.isfinite(got["y_out"]).all() and np.isfinite(got["u"]).all()
    assert (np.diff(c["indptr"])[5] == 0) and (got["grad"][:, 5] == -4.0 * c["F"][:, 5] / got["Z"]).all(), "an empty row: the repulsion alone"


def test_two_calls_agree_bit_for_bit_and_the_optional_outputs_change_nothing(dev):
    c = R.update_case(D=2)
    a, b, bare = _call(dev, c), _call(dev, c), _call(dev, c, with_outputs=False)
    for k in ("y_out", "u", "gain", "kl_row", "grad"):
        assert np.array_equal(a[k], b[k]), k
    assert a["Z"] == b["Z"] == bare["Z"]
    for k in ("y_out", "u", "gain"):
        assert np.array_equal(a[k], bare[k]), k


def test_kl_of_the_reference_layout(dev):
    """sum(kl_row) + log Z is the KL divergence of the layout: against the dense float64 one"""
    c = R.update_case(D=2)
    got = _call(dev, c)
    P = R.dense_p(c["indptr"], c["cols"], c["vals"], c["n"])
    r = R.update_ref(c)
    assert abs(got["kl_row"].sum() + np.log(got["Z"]) - R.kl_ref(c["y"], P)) <= r["e_kl"].sum() + 1e-12


def test_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.tsne_ops import update
    c = R.update_case(D=2)
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("indptr", "cols", "vals", "y", "u", "gain", "Zrow", "F")}
    Z = torch.zeros(1, dtype=torch.float64, device=dev)
    with pytest.raises(_abi.SpvError, match="y_out must not be y_in"):
        update(t["y"], t["y"], t["indptr"], t["cols"], t["vals"], t["Zrow"], t["F"], Z, t["u"], t["gain"], 1.0, 0.5, 100.0)
    with pytest.raises(_abi.SpvError, match="indptr"):
        update(t["y"], torch.empty_like(t["y"]), t["indptr"][:-1], t["cols"], t["vals"], t["Zrow"], t["F"], Z, t["u"], t["gain"], 1.0, 0.5, 100.0)
    with pytest.raises(_abi.SpvError, match="F"):
        update(t["y"], torch.empty_like(t["y"]), t["indptr"], t["cols"], t["vals"], t["Zrow"], t["F"].float(), Z, t["u"], t["gain"], 1.0, 0.5, 100.0)
