"""Every log line and info() of the six spin front-end classes against tests/golden/spin_frontend_logs.json, the record of the
commit before they shared spin_frontend.hpp (scripts/record_spin_frontend_logs.py): the refusals (no model, no state, a state of
the wrong length, a zero state, a product state outside the sites or the sector, Krylov dimension 1, a dt that is not finite, a
tolerance that is not positive, coefficient lists of the wrong length or with a NaN in each class's wording, S+ of the sector with
every site up and S- of the empty one), a site operator that annihilates the state exactly, the note of a run that starts again
in the middle, and one successful call of each class, on the open chain of 4 sites and the ring of 6 sites with 3 up.  Lines are
compared as text, whole; the two kinds that print a floating-point number ("sub-steps: ..." and "lanczos steps: ...") too."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import spin_frontend_log_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_log_line_is_the_recorded_one(tmp_path):
    with open(cases.FIXTURE) as f:
        recorded = json.load(f)
    seen = cases.run(tmp_path)
    assert [c["case"] for c in seen] == [c["case"] for c in recorded]
    assert len(recorded) == 154 and sum(len(c["log"]) for c in recorded) == 308
    different = [(s["case"], s["info"], s["log"], r["info"], r["log"]) for s, r in zip(seen, recorded) if s != r]
    for d in different:
        print(d)
    assert not different
