"""CPU: tests/launch_paths.py against the HIP sources.  The caps and workgroup sizes in the table are the ones in
noise_robust_vit_amd/csrc/*.hip, and every shape test_launch_paths_gpu.py runs makes its kernel walk its grid-stride loop for
two full passes and a partial one.  A cap raised later fails here, by the record's name."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import launch_paths as LP  # noqa: E402

NAMES = [r.name for r in LP.TABLE]


def test_the_table_names_every_entry_point_once():
    assert len(set(NAMES)) == len(NAMES)
    for r in LP.TABLE:
        assert os.path.exists(os.path.join(LP.CSRC, r.source)), r.source
        assert r.threshold == r.cap * r.group and r.threshold_elements == r.threshold * r.per_item
    assert set(LP.ALSO_WRAPPED) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_table_agrees_with_the_source_and_the_shape_wraps(name):
    rec = LP.get(name)
    found = LP.problems(rec, LP.source_text(rec))
    assert found == [], "\n".join(found)
    for shape in LP.shapes_of(rec):
        items = rec.items(shape)
        assert items >= LP.MIN_PASSES * rec.threshold, (name, shape, items, rec.threshold)
        assert items % rec.threshold != 0, (name, shape, items, rec.threshold)


@pytest.mark.parametrize("name", NAMES)
def test_a_doubled_cap_is_reported_by_name(name):
    """The check itself: with the record's cap at twice its value in (a copy of the text of) the source, the comparison fails
    and says which record.  Nothing is written anywhere."""
    rec = LP.get(name)
    text = LP.source_text(rec)
    changed = LP.doubled_cap(rec, text)
    assert changed != text
    found = LP.problems(rec, changed)
    assert found and all(f.startswith(name + ":") for f in found), found
    assert any(str(2 * rec.cap) in f for f in found), found
    # at twice the cap the committed shape would make little more than one pass: that is reported too
    assert any("passes of" in f for f in found), found


def test_layernorm_widths_reach_the_dispatch_cases_the_issue_names():
    """ln_lpr / ln_maxj of nrv_norm.hip, re-computed: the widths of the wrapped LayerNorm cases launch J = 6 and J = 8 of the
    64-lane form, leave the last chunk of a lane partly empty, and leave lanes of a 32-lane half-wave idle."""
    steps = (1, 2, 3, 4, 5, 6, 8, 16)
    text = LP.source_text(LP.get("layernorm_fwd"))
    assert "static const int steps[8] = {1, 2, 3, 4, 5, 6, 8, 16};" in text
    assert "const int chunks = (dim / 4 + lpr - 1) / lpr;" in text
    got = {}
    for dim in LP.LN_DIMS:
        lpr = 32 if dim <= 512 else 64
        chunks = (dim // 4 + lpr - 1) // lpr
        got[dim] = (lpr, next(s for s in steps if chunks <= s))
    assert got == LP.LN_DIMS
    js = {j for lpr, j in got.values() if lpr == 64}
    assert {6, 8, 16} <= js
    assert any(lpr == 64 and dim // 4 < lpr * j for dim, (lpr, j) in got.items())       # guards `c < dim` do the work
    assert any(lpr == 32 and dim // 4 < lpr for dim, (lpr, j) in got.items())           # idle lanes in a half-wave
    for name in ("layernorm_fwd_half_wave", "layernorm_bwd_half_wave", "layernorm_fwd", "layernorm_bwd"):
        rows = LP.get(name).wrapped["rows"]
        assert rows % 2 == 1 and rows % 4 in (1, 3), (name, rows)
