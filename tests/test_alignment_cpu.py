"""Completeness of the alignment sweep (tests/test_gpu_alignment.py), checked without a GPU: every `dsa_*_fwd` / `dsa_*_bwd` entry of
include/diffsptk_amd.h and every public module is named by the sweep's table (tests/alignment_rows.py) or exempt there with a reason."""
import inspect
import re

import torch

from alignment_rows import EXEMPT, NOT_A_MODULE, ROWS
from diffsptk_amd import _lib
from diffsptk_amd import modules as nn


def _entries():
    signatures, _ = _lib.parse_header(open(_lib.HEADER).read())
    return {name for name in signatures if re.fullmatch(r"dsa_\w+_(fwd|bwd)", name)}


def test_every_entry_is_swept_or_exempt():
    entries = _entries()
    assert len(entries) > 60   # the pattern still finds the header's entries
    claimed = {name for row in ROWS.values() for name in row}
    assert claimed <= entries, f"the table names entries the header does not have: {sorted(claimed - entries)}"
    assert set(EXEMPT) <= entries, f"exemptions for entries the header does not have: {sorted(set(EXEMPT) - entries)}"
    assert not claimed & set(EXEMPT), f"both swept and exempt: {sorted(claimed & set(EXEMPT))}"
    missing = entries - claimed - set(EXEMPT)
    assert not missing, f"no row of tests/alignment_rows.py names {sorted(missing)}: add them to a row of the sweep (or to EXEMPT, with a reason)"
    assert all(isinstance(reason, str) and len(reason.split()) >= 3 for reason in EXEMPT.values())
    assert len(EXEMPT) <= 5   # an exemption is an exception


def test_every_public_module_has_a_row():
    classes = set()
    for name in nn.__all__:
        obj = getattr(nn, name)
        if name in NOT_A_MODULE:
            continue
        assert inspect.isclass(obj) and issubclass(obj, torch.nn.Module), name
        classes.add(obj.__name__)   # (an alias names its class)
    assert classes == set(ROWS), f"without a row: {sorted(classes - set(ROWS))}; rows of no module: {sorted(set(ROWS) - classes)}"
    assert set(NOT_A_MODULE) <= set(nn.__all__)
