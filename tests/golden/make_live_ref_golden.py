"""tests/golden/live_ref.npz: what the REFERENCE builds under oracle/_ref answer in the tests that compare the CPU restatement with
them live -- tests/test_oracle_nn.py (hecmw_solve: other methods, SCALING=YES), tests/test_oracle_nl.py::test_elements_vs_reference
(ref_nl) and tests/test_oracle_update.py::test_oracle_update_linear_equals_reference_build (ref_update).  Those tests run the
binaries where they exist and fall back on these answers elsewhere.  Same inputs as the tests (their own case builders).
Run where the reference sources are available, after `python oracle/build_ref.py`."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from nn_cases import nn_system                                      # noqa: E402
from oracle import refrun                                           # noqa: E402
import test_oracle_nl as tnl                                        # noqa: E402
import test_oracle_nn as tnn                                        # noqa: E402
import test_oracle_update as tup                                    # noqa: E402

out = {}
for scaling, nds, cases in ((False, (1, 6), tnn.OTHER_METHODS), (True, (1, 2, 4, 5, 6), tnn.SCALING_CASES)):
    for nd in nds:
        A = nn_system(nd)
        for meth, pc, thr in cases:
            I, R = refrun.default_params(method=meth, precond=pc)
            if scaling:
                I[6] = 1
            r = refrun.run_solve(A, I, R, threads=thr)
            tag = tnn.live_tag(nd, meth, pc, thr, scaling)
            out[tag + "iter"], out[tag + "X"] = np.int32(r["iter"]), r["X"]
            print(tag, r["iter"])
for name in tnl.materials():
    mat, m, unode, dunode, st = tnl.element_case(name, seed=3)
    ke0, qf, ke1, rst = refrun.run_nl_elements(mat, m.coord, m.conn, unode, dunode, st)
    t = "nl_%s_" % name
    out[t + "ke0"], out[t + "qf"], out[t + "ke1"] = ke0, qf, ke1
    for k in tnl.NL_STATE_KEYS:
        out[t + k] = rst[k]
    print(t, np.abs(ke0).max())
for eo in (1, 2, 3):
    m, u, du = tup.update_case(eo)
    for k, v in zip(("strain", "stress", "qforce"), refrun.run_update(eo, m.coord, m.conn, 210000.0, 0.3, u, du)):
        out["upd%d_%s" % (eo, k)] = v
    print("upd%d" % eo)
np.savez_compressed(os.path.join(HERE, "live_ref.npz"), **out)
