"""The CLI mirror's --compress_outputs {none,rows,ring} (a dctfhe addition, default none): it parses, maps onto
Configuration(compress_output_ciphertexts=...), and leaves the reference's flags and defaults where they were."""
import importlib.util
import os
import sys

import pytest

from test_cli_flags import REFERENCE_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec = importlib.util.spec_from_file_location("he_cli_ring", os.path.join(ROOT, "dct-cryptonets_amd", "homomorphic_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flag_parses_and_reference_defaults_stay(monkeypatch):
    from dctfhe.quantized_module import Configuration
    mod = _cli()
    monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py"])
    ns = vars(mod.parse_args())
    assert ns["compress_outputs"] == "none"
    for k, v in REFERENCE_FLAGS.items():
        assert k in ns and ns[k] == v, (k, ns.get(k), v)
    for value, form in (("none", False), ("rows", True), ("ring", "ring")):
        monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py", "--compress_outputs", value, "--fhe_mode", "execute"])
        ns = vars(mod.parse_args())
        assert ns["compress_outputs"] == value and ns["fhe_mode"] == "execute"
        assert Configuration(compress_output_ciphertexts=ns["compress_outputs"]).compress_output_ciphertexts == form
    monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py", "--compress_outputs", "glwe"])
    with pytest.raises(SystemExit):
        mod.parse_args()
