"""CPU: the host side of token suppression (csrc/suppress.hpp through AX_WHISPER_NonSpeechTokens and AX_WHISPER_ConfigSuppressTokens,
tools/modelgen.py and tools/convert_weights.py) against tests/suppress_reference.py and the published list. No GPU and no model."""
import json
import os

import pytest

import suppress_reference as sup
from conftest import GOLDEN

TABLE_PATH = os.path.join(GOLDEN, "multilingual.tiktoken")
NV, EOT, T = 51865, 50257, 50364


@pytest.fixture(scope="module")
def fixture_ids():
    return json.load(open(os.path.join(GOLDEN, "non_speech_multilingual.json")))


@pytest.fixture(scope="module")
def tokens_file(tmp_path_factory):
    import modelgen

    p = str(tmp_path_factory.mktemp("suppress_tokens") / "micro-tokens.txt")
    modelgen.write_tokens(p, TABLE_PATH)
    return p


def _config(tmp_path, value, name="c.json", **over):
    import modelgen

    cfg = modelgen.make_config("micro", modelgen.DIMS["micro"])
    assert (cfg["n_vocab"], cfg["eot"], cfg["no_timestamps"] + 1) == (NV, EOT, T)
    if value is not None:
        cfg["suppress_tokens"] = value
    cfg.update(over)
    p = tmp_path / name
    p.write_text(json.dumps(cfg))
    return str(p)


def test_non_speech_tokens_of_a_written_tokens_file(built_lib, tokens_file, fixture_ids):
    assert built_lib.non_speech_tokens(tokens_file) == fixture_ids
    assert built_lib.non_speech_tokens(tokens_file) == sup.non_speech_tokens(sup.load_ranks(tokens_file))


def test_non_speech_tokens_refuse_a_table_without_the_bytes(built_lib, tmp_path):
    import modelgen

    p = str(tmp_path / "synthetic-tokens.txt")
    modelgen.write_tokens(p, None)  # rank i -> "t{i} ": no entry for a single byte
    with pytest.raises(RuntimeError, match="no entry for a byte"):
        built_lib.non_speech_tokens(p)
    with pytest.raises(RuntimeError, match="cannot open"):
        built_lib.non_speech_tokens(str(tmp_path / "missing.txt"))


def test_config_key_parses(built_lib, tmp_path, tokens_file, fixture_ids):
    cs = built_lib.config_suppress_tokens
    assert cs(_config(tmp_path, None), tokens_file) == []
    assert cs(_config(tmp_path, None)) == []
    assert cs(_config(tmp_path, [])) == []
    assert cs(_config(tmp_path, [-1]), tokens_file) == fixture_ids
    assert cs(_config(tmp_path, [7, 3, 3, EOT + 1, T - 1])) == [3, 7, EOT + 1, T - 1]  # no tokens file needed without -1
    mixed = cs(_config(tmp_path, [11, -1, 50000, -1, 1]), tokens_file)
    assert mixed == sorted(set(fixture_ids) | {11, 50000})
    assert mixed == sup.check_ids(fixture_ids + [11, 50000, 1], NV, EOT, T)


@pytest.mark.parametrize("value, text", [([EOT], "eot"), ([T], "timestamp id"), ([NV - 1], "timestamp id"), ([NV], "outside the vocabulary"),
                                         ([-2], "list of ids"), ([1.5], "list of ids"), (["1"], "list of ids"), (7, "list of ids"),
                                         ({"a": 1}, "list of ids"), ([[1, 2]], "list of ids")],
                         ids=["eot", "first_timestamp", "last_timestamp", "past_the_vocabulary", "below_minus_one", "fraction", "string",
                              "number", "object", "nested"])
def test_config_key_refusals_give_a_text(built_lib, tmp_path, tokens_file, value, text):
    with pytest.raises(RuntimeError, match=text):
        built_lib.config_suppress_tokens(_config(tmp_path, value), tokens_file)


def test_config_minus_one_needs_a_usable_tokens_file(built_lib, tmp_path):
    import modelgen

    with pytest.raises(RuntimeError, match="no tokens file"):
        built_lib.config_suppress_tokens(_config(tmp_path, [-1]))
    p = str(tmp_path / "synthetic-tokens.txt")
    modelgen.write_tokens(p, None)
    with pytest.raises(RuntimeError, match="no entry for a byte"):
        built_lib.config_suppress_tokens(_config(tmp_path, [-1]), p)


def test_modelgen_writes_the_key(built_lib, tmp_path, fixture_ids):
    import modelgen

    assert modelgen.parse_suppress_tokens(None) is None
    assert modelgen.parse_suppress_tokens("-1") == [-1] and modelgen.parse_suppress_tokens("1,2, 3") == [1, 2, 3]
    dims = modelgen.DIMS["micro"]
    d = modelgen.write_model_dir(str(tmp_path), "micro", dims, weights=modelgen.synth_weights(dims, 3), tiktoken_path=TABLE_PATH,
                                 suppress_tokens=[-1])
    assert json.load(open(os.path.join(d, "micro_config.json")))["suppress_tokens"] == [-1]
    assert built_lib.config_suppress_tokens(os.path.join(d, "micro_config.json"), os.path.join(d, "micro-tokens.txt")) == fixture_ids


def test_convert_weights_copies_the_suppress_tokens(built_lib, tmp_path):
    """tools/convert_weights.py --hf: generation_config.json's suppress_tokens arrive in the model's config file, special ids between
    eot and the timestamps included, and the engine's reader takes them from there"""
    import convert_weights
    import modelgen

    hf = tmp_path / "hf"
    hf.mkdir()
    assert convert_weights.hf_suppress_tokens(str(hf)) is None  # no generation_config.json
    (hf / "generation_config.json").write_text(json.dumps({"max_length": 448}))
    assert convert_weights.hf_suppress_tokens(str(hf)) is None  # no key
    listed = [1, 2, 7, 359, 50254, 50258, 50358, 50359, 50360, 50361, 50362]
    (hf / "generation_config.json").write_text(json.dumps({"suppress_tokens": listed}))
    assert convert_weights.hf_suppress_tokens(str(hf)) == listed
    assert convert_weights.hf_suppress_tokens(str(hf / "model.safetensors")) == listed  # beside a weights file
    dims = modelgen.DIMS["micro"]
    d = convert_weights.write_model(modelgen.synth_weights(dims, 3), "micro", str(tmp_path / "m"), "BF16", TABLE_PATH,
                                    suppress_tokens=convert_weights.hf_suppress_tokens(str(hf)))
    assert json.load(open(os.path.join(d, "micro_config.json")))["suppress_tokens"] == listed
    assert built_lib.config_suppress_tokens(os.path.join(d, "micro_config.json")) == listed
    d = convert_weights.write_model(modelgen.synth_weights(dims, 3), "micro", str(tmp_path / "n"), "BF16", TABLE_PATH)
    assert "suppress_tokens" not in json.load(open(os.path.join(d, "micro_config.json")))
    (hf / "generation_config.json").write_text(json.dumps({"suppress_tokens": [[1, 2]]}))
    with pytest.raises(ValueError):
        convert_weights.hf_suppress_tokens(str(hf))
