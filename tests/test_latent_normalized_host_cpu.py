"""CPU: the host side of the normalised latents -- the signature of get_latent_representation, and the refusal of the Monte-Carlo
mean (normalized=True, give_mean=True), which is not built, before any device work.  No GPU calls."""
import inspect

import pytest


def test_monte_carlo_mean_is_refused_before_any_device_work():
    """get_latent_representation refuses before it touches the model: called on an object that has no model at all it must
    still raise the NotImplementedError (anything else would be an AttributeError)."""
    from spvipes_amd.model import spVIPES
    with pytest.raises(NotImplementedError, match="give_mean"):
        spVIPES.get_latent_representation(object(), [[0], [1]], normalized=True)
    with pytest.raises(NotImplementedError, match="give_mean"):
        spVIPES.get_latent_representation(object(), [[0], [1]], normalized=True, give_mean=True, mc_samples=100)


def test_sampled_normalized_latents_are_not_refused():
    """normalized=True, give_mean=False passes the argument check and goes on to the model (an object without one: AttributeError)"""
    from spvipes_amd.model import spVIPES
    with pytest.raises(AttributeError):
        spVIPES.get_latent_representation(object(), [[0], [1]], normalized=True, give_mean=False)


def test_signature_keeps_the_reference_parameters():
    from spvipes_amd.model import spVIPES
    sig = inspect.signature(spVIPES.get_latent_representation)
    names = list(sig.parameters)
    reference = ["self", "group_indices_list", "adata", "indices", "normalized", "give_mean", "mc_samples", "batch_size", "drop_last"]   # model/spvipes.py:425-435
    assert names[:len(reference)] == reference
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["adata"], d["indices"], d["normalized"], d["give_mean"], d["mc_samples"], d["batch_size"], d["drop_last"]) == (None, None, False, True, 5000, None, None)
    for k in reference[1:]:
        assert sig.parameters[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
