"""CPU: the decoder's operand-layout choice (spVIPESmodule(decoder_slots=...)): the limit arithmetic of the narrow (16 / 32 K slots)
and wide (32 / 64) layouts, the parameter shapes the reference builds, the zero default of the C ABI's kslots fields, and the
oracle against the reference runs of wide-layout shapes (tests/golden/wide/*.npz, tests/golden/make_wide_goldens.py)."""
import ctypes
import glob
import os

import pytest
import torch

from spvipes_amd import _abi
from spvipes_amd.module import spVIPESmodule, decoder_layout


def _mod(nb, slots=None, n_s=25, n_p=10, G=(50, 40), H=128):
    kw = {} if slots is None else {"decoder_slots": slots}
    return spVIPESmodule({0: G[0], 1: G[1]}, use_labels=True, n_batch=nb, n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p, **kw)


def test_narrow_is_the_default_and_still_refuses_nine_categories():
    with pytest.raises(NotImplementedError, match="wide"):   # (the message names the wide option)
        _mod(9)
    with pytest.raises(NotImplementedError, match="private regressor"):
        _mod(9, "narrow")
    assert _mod(5).dec_slots == _abi.DEC_NARROW


@pytest.mark.parametrize("slots", ["auto", "wide"])
def test_wide_layout_takes_fourteen_categories_and_refuses_fifteen(slots):
    m = _mod(14, slots)
    assert m.dec_slots == _abi.DEC_WIDE
    assert all(d.dec_slots == _abi.DEC_WIDE for d in m.decoders.values())
    with pytest.raises(NotImplementedError, match="mixture GEMM"):
        _mod(15, slots)
    # smaller latents: the mixture GEMM binds at 24 categories
    _mod(24, slots, n_s=10, n_p=5)
    with pytest.raises(NotImplementedError, match="mixture GEMM"):
        _mod(25, slots, n_s=10, n_p=5)


def test_bad_decoder_slots_value():
    with pytest.raises(ValueError):
        _mod(3, "medium")


def test_auto_picks_narrow_wherever_narrow_fits():
    for n_s in range(1, 32):
        for n_p in range(1, 16):
            for nb in range(0, 16):
                n_cov = nb if nb > 1 else 0
                try:
                    want = decoder_layout("narrow", n_p, n_s, n_cov)
                except NotImplementedError:
                    continue
                assert decoder_layout("auto", n_p, n_s, n_cov) == want == _abi.DEC_NARROW, (n_s, n_p, nb)
    assert decoder_layout("auto", 10, 25, 6) == _abi.DEC_WIDE   # the first shape narrow refuses at 25 / 10
    assert decoder_layout("auto", 3, 6, 13) == _abi.DEC_WIDE    # only the private regressor is too narrow


@pytest.mark.parametrize("nb", [6, 12, 14])
def test_wide_parameter_shapes_are_the_references(nb):
    G, H, n_s, n_p = (50, 40), 64, 25, 10
    m = _mod(nb, "auto", G=G, H=H)
    for g in range(2):
        for kind, n in (("shared", n_s), ("private", n_p)):
            assert m.encoders[g][kind].fc1.weight.shape == (H, G[g] + nb)
        d = m.decoders[g]
        assert d.factor_regressor_private.linear.weight.shape == (G[g], n_p + nb)
        assert d.factor_regressor_shared.linear.weight.shape == (G[g], n_s + nb)
        assert d.sigmoid_decoder.linear.weight.shape == (256, n_s + n_p + nb)
        assert d.mixture.linear.weight.shape == (G[g], 256 + n_s + n_p + nb)


def test_abi_layout_fields_default_to_the_narrow_layout():
    for cls in (_abi.SpvDecParams, _abi.SpvZsplitArgs, _abi.SpvFoldBatch):
        assert cls().kslots == 0
        assert cls._fields_[-1] == ("kslots", ctypes.c_int32)   # trailing: zero-initialised callers keep their layout
    assert _abi.DEC_NARROW == (0, 16, 32, 48) and _abi.DEC_WIDE == (1, 32, 64, 96)


def test_narrow_module_decoders_report_the_narrow_layout():
    from spvipes_amd.dec_ops import dec_slots
    m = _mod(3)
    assert all(dec_slots(d).kslots == 0 for d in m.decoders.values())
    assert dec_slots(object()) == _abi.DEC_NARROW   # a decoder built without the attribute


WIDE_CASES = sorted("wide/" + os.path.splitext(os.path.basename(p))[0]
                    for p in glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide", "*.npz")))


def test_wide_fixtures_exist_and_need_the_wide_layout():
    from tests._golden import Golden
    assert len(WIDE_CASES) == 4, WIDE_CASES
    for case in WIDE_CASES:
        g = Golden(case)
        assert g.n_batch > 5 and decoder_layout("auto", g.n_p, g.n_s, g.n_batch) == _abi.DEC_WIDE, case
        with pytest.raises(NotImplementedError):
            decoder_layout("narrow", g.n_p, g.n_s, g.n_batch)


@pytest.mark.parametrize("case", WIDE_CASES)
def test_oracle_matches_wide_reference_runs(case):
    """the checks tests/test_oracle_vs_golden.py makes of the narrow fixtures, on the wide ones"""
    from tests import test_oracle_vs_golden as T
    T.test_inference_stats_match_reference(case)
    T.test_loss_terms_match_reference(case)
    T.test_gradients_match_reference(case)
    if "train" in case:
        T.test_running_stats_match_reference(case)
    T.test_loadings_match_reference(case)


def test_auto_leaves_shapes_without_covariates_on_the_narrow_layout():
    """"auto" widens only for covariate columns: without covariates a latent size the narrow kernels do not take is still reported"""
    assert decoder_layout("auto", 20, 25, 0) == _abi.DEC_NARROW
    assert decoder_layout("wide", 20, 25, 0) == _abi.DEC_WIDE   # (asked for explicitly)

