"""The one keyword path of the generation options: the entries' option parameters are `parse_request`'s keyword-only ones
(names, order, defaults), and every option a caller passes arrives in `parse_request` under its own name."""
import inspect

import pytest

from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd.conformer_generator import MLConformerGenerator

ENTRIES = ("generate_conformers", "generate_conformers_sharded", "forward")


def _keyword_only():
    return [p for p in inspect.signature(postprocess.parse_request).parameters.values()
            if p.kind is inspect.Parameter.KEYWORD_ONLY]


def test_parse_request_takes_its_options_by_keyword_only():
    params = list(inspect.signature(postprocess.parse_request).parameters.values())
    assert [p.name for p in params[:2]] == ["gen", "reference_conformer"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[2:])
    assert postprocess.REQUEST_KEYWORDS == tuple(p.name for p in params[2:])
    assert postprocess.REQUEST_KEYWORDS[0] == "reference_context" and len(postprocess.REQUEST_KEYWORDS) == 37
    with pytest.raises(TypeError):
        postprocess.parse_request(object(), None, True)


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_entries_spell_the_options_as_parse_request_does(entry):
    params = list(inspect.signature(getattr(MLConformerGenerator, entry)).parameters.values())
    names = [p.name for p in params]
    options = params[names.index("shape_scores"):]             # the options close the signature, behind `sample_seed`
    assert names[names.index("shape_scores") - 1] == "sample_seed"
    want = [p for p in _keyword_only() if p.name != "reference_context"]
    assert [(p.name, p.default) for p in options] == [(p.name, p.default) for p in want]
    context = inspect.signature(postprocess.parse_request).parameters["reference_context"]
    assert params[names.index("reference_context")].default is context.default is None


class _Arrived(Exception):
    pass


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_option_arrives_under_its_own_name(entry, monkeypatch):
    seen = {}
    defaults = {p.name: p.default for p in _keyword_only()}

    def parse(gen, reference_conformer, **keywords):
        seen.update(keywords, reference_conformer=reference_conformer, gen=gen)
        raise _Arrived                                         # in front of any device work

    monkeypatch.setattr(postprocess, "parse_request", parse)
    gen = MLConformerGenerator.__new__(MLConformerGenerator)
    conformer = object()
    for name in postprocess.REQUEST_KEYWORDS:
        sentinel = object()
        seen.clear()
        with pytest.raises(_Arrived):
            getattr(gen, entry)(reference_conformer=conformer, **{name: sentinel})
        assert seen.pop("gen") is gen and seen.pop("reference_conformer") is conformer
        assert set(seen) == set(postprocess.REQUEST_KEYWORDS)
        assert seen[name] is sentinel
        assert all(seen[other] is defaults[other] or seen[other] == defaults[other]
                   for other in postprocess.REQUEST_KEYWORDS if other != name), name
