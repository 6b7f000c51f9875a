"""optim.Adafactor's constructor surface and the cfm_adafactor_step_ex binding, without a GPU."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _param():
    return torch.nn.Parameter(torch.zeros(4, 3))


@pytest.mark.parametrize("kw", [dict(), dict(weight_decay=0.1), dict(capturable=True),
                                dict(lr=1e-3, relative_step=False, scale_parameter=True)],
                         ids=["defaults", "weight_decay", "capturable", "scale_parameter"])
def test_constructor_accepts_transformers_options(kw):
    from nn_conformer_for_speech_recognition_amd.optim import Adafactor
    opt = Adafactor([_param()], **kw)
    group = opt.param_groups[0]
    assert group["scale_parameter"] is True
    assert group["capturable"] is kw.get("capturable", False)
    assert group["weight_decay"] == kw.get("weight_decay", 0.0)


def test_constructor_defaults_are_transformers():
    import inspect
    from transformers import Adafactor as HFAdafactor
    from nn_conformer_for_speech_recognition_amd.optim import Adafactor
    ours = inspect.signature(Adafactor.__init__).parameters
    for name, p in inspect.signature(HFAdafactor.__init__).parameters.items():
        assert name in ours and ours[name].default == p.default, name
    assert ours["capturable"].default is False


def test_value_errors_still_raise():
    from nn_conformer_for_speech_recognition_amd.optim import Adafactor
    with pytest.raises(ValueError, match="manual `lr`"):
        Adafactor([_param()], lr=1e-3, relative_step=True)
    with pytest.raises(ValueError, match="warmup_init"):
        Adafactor([_param()], lr=1e-3, relative_step=False, warmup_init=True)


def test_state_dict_without_capturable_key_loads():
    """A state dict written before the keyword existed (or by transformers) has no group["capturable"]."""
    from nn_conformer_for_speech_recognition_amd.optim import Adafactor
    opt = Adafactor([_param()])
    sd = opt.state_dict()
    del sd["param_groups"][0]["capturable"]
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["capturable"] is False


def test_step_ex_prototype_and_struct():
    from nn_conformer_for_speech_recognition_amd import _lib
    res, args = _lib._SIGS["cfm_adafactor_step_ex"]
    old_res, old_args = _lib._SIGS["cfm_adafactor_step"]
    assert res is ctypes.c_int and len(args) == 14
    assert args[:10] == old_args[:10]               # the same table, task totals and buffers
    # the struct mirrors the header's field order, and the flags its enum
    src = open(os.path.join(REPO, "include", "cfm.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} cfm_adafactor_hyper;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip(" *") for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.AdafactorHyper._fields_]
    enum = dict(re.findall(r"CFM_ADA_([A-Z_]+) = 1 << (\d)", src))
    assert {k: 1 << int(v) for k, v in enum.items()} == {
        "SCALE_PARAMETER": _lib.ADA_SCALE_PARAMETER, "RELATIVE_STEP": _lib.ADA_RELATIVE_STEP,
        "WARMUP_INIT": _lib.ADA_WARMUP_INIT, "DEVICE_STEP": _lib.ADA_DEVICE_STEP}
    assert ctypes.sizeof(_lib.AdafactorHyper) == 8 + 7 * 4 + 4 + 2 * 8


def test_step_ex_validates_on_the_host():
    """The argument checks come before any launch, so they can be seen without a GPU."""
    from nn_conformer_for_speech_recognition_amd import _lib as L
    args = (None, 0, 0, 0, 0, 0, 0, None, None, None, None, None)
    with pytest.raises(L.CfmError, match="null hyper"):
        L.call("cfm_adafactor_step_ex", *args, None, None)
    h = L.AdafactorHyper(flags=L.ADA_DEVICE_STEP)
    with pytest.raises(L.CfmError, match="device step without"):
        L.call("cfm_adafactor_step_ex", *args, ctypes.byref(h), None)
    h = L.AdafactorHyper(flags=L.ADA_SCALE_PARAMETER)
    with pytest.raises(L.CfmError, match="scale_parameter without"):
        L.call("cfm_adafactor_step_ex", *args, ctypes.byref(h), None)
    h = L.AdafactorHyper(weight_decay=0.1)
    with pytest.raises(L.CfmError, match="bad args"):
        L.call("cfm_adafactor_step_ex", *args, ctypes.byref(h), None)
