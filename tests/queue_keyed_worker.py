"""Child process of test_queue_keyed.py / test_queue_keyed_gpu.py: one parity run against the oracle (tests/parity.py)
in a fresh process, so the knobs in its environment (CCMI_QUEUE_KEYED, CCMI_QUEUE_KEYED_STRIDE, CCMI_PROFILE, ...) are the
ones the library reads when it starts. The session's CCMI_PROFILE counters go to stderr when the session closes; the
parent reads them from there. Prints "parity ok" after the comparison.

usage: queue_keyed_worker.py emu|gpu <case name>"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "cruise-control_amd"))
sys.path.insert(0, HERE)

import ccmi  # noqa: E402
from oracle_binding import Oracle  # noqa: E402
from parity import check_product_against_oracle  # noqa: E402

CASES = {
    "b20_default": (dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300), "default"),
    "b300_c1": (dict(num_racks=8, num_brokers=300, num_replicas=30000, num_topics=1000), "c1"),
    "b300_default": (dict(num_racks=8, num_brokers=300, num_replicas=30000, num_topics=1000), "default"),
    "dead2": (dict(num_racks=5, num_brokers=10, num_replicas=3000, num_topics=100, num_dead_brokers=2), "default"),
}


def main():
    which, case = sys.argv[1], sys.argv[2]
    path = os.path.join(REPO, "tests", "emu", "libccmi_emu.so") if which == "emu" else \
        os.path.join(REPO, "cruise-control_amd", "libccmi.so")
    lib = ccmi.Library.get(path)
    Oracle.lib()
    props, goals = CASES[case]
    goals = list(ccmi.C1_GOALS) if goals == "c1" else list(ccmi.DEFAULT_GOALS)
    cm, res, oc = check_product_against_oracle(lib, props, goals, 1.05)
    print("parity ok", len(cm.actions()), "actions")
    del cm, res, oc  # closes the session: the profile is printed then


if __name__ == "__main__":
    main()
