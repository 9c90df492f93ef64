"""hddm_amd — MI355X-native WFPT likelihood engine for HDDM.

`hddm_amd.wfpt` is the drop-in for the reference's `wfpt` extension module
(src/wfpt.pyx); `hddm_amd.likelihoods` carries the PyMC-facing `wfpt_like`
(hddm/likelihoods.py:52-73). All densities come from the HIP kernels in
hddm_amd/csrc (libwfpt_amd.so); importing `hddm_amd.wfpt` without the built
library raises ImportError.

The model classes are reached through the package, loaded on first use (they
import `hddm_amd.wfpt`): HDDM, HDDMChains, HDDMRegressor, HDDMrl,
HDDMrlRegressor.
"""
__version__ = "0.1.0"

_MODELS = {"HDDM": "hierarchical", "HDDMChains": "hierarchical", "HDDMRegressor": "regression",
           "HDDMrl": "rl", "HDDMrlRegressor": "rl_regression"}


def __getattr__(name):
    if name in _MODELS:
        import importlib
        return getattr(importlib.import_module(f".{_MODELS[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
