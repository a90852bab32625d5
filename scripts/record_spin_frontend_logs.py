"""Records tests/golden/spin_frontend_logs.json: every log line and info() that tests/cpp/spin_frontend_logs_amd.cpp draws from the
spin front-end classes of the checked-out headers.  It was run once, on the GPU, at the commit before spin_frontend.hpp existed;
tests/test_gpu_spin_frontend_logs.py holds every later build to that record line for line.  Run it again only to extend the
cases, and then from a commit whose log lines are known to be right.

    python scripts/record_spin_frontend_logs.py [OUT.json]
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import spin_frontend_log_cases as cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else cases.FIXTURE
    with tempfile.TemporaryDirectory() as tmp:
        recorded = cases.run(tmp)
    with open(out, "w") as f:
        json.dump(recorded, f, indent=1)
        f.write("\n")
    print(f"{len(recorded)} cases, {sum(len(c['log']) for c in recorded)} lines -> {out}")
