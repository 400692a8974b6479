"""worker of tests/test_gpu_thin.py::test_thinned_run_of_two_ranks_sharing_one_gpu: thinned calls on
an ensemble shared by two ranks (two processes on the one GPU of the test box).  The block of such a
call stays full-rate in HBM, is merged over the ranks on the host and sliced there."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["NAIMA_AMD_DEVICE"] = "0"  # both ranks share the one GPU of the test box
import naima_amd as na  # noqa: E402
from bench import build_problem  # noqa: E402
from naima_amd.dist import HostComm  # noqa: E402
from naima_amd.sampler import EnsembleSampler  # noqa: E402

out, name, nw = sys.argv[1], sys.argv[2], int(sys.argv[3])
comm = HostComm()  # (RCCL refuses two ranks on one GPU; the shared loop needs the control plane only)
model, p0, raw, data, prior, labels = build_problem(name, na)
nd = p0.size
s = EnsembleSampler(nw, nd, na.lnprob, args=[data, model, prior], seed=42, comm=comm,
                    naima_style=True, store_blobs=True, device=True, nan_policy="reject")
pos = p0 * (1 + 0.003 * np.random.default_rng(1).standard_normal((nw, nd)))
st = s.run_mcmc(pos, 5)               # warm-up and plan
st = s.run_mcmc(st, 14, thin_by=5)    # 70 steps: three launches of the shared loop
dev = s._dev
assert dev.shared and dev.resident_launches >= 3, (dev.shared, getattr(dev, "resident_reason", None))
assert dev.thin_info["where"] == "host" and dev.thin_info["thin_by"] == 5
assert dev.hist[-1]["thin_by"] == 5 and dev.hist[-1]["coords"].shape[0] == 70
st = s.run_mcmc(st, 3, store=False, thin_by=3)
st = s.run_mcmc(st, 4)
st = s.run_mcmc(st, 2, thin_by=33)
assert s.iteration == 5 + 14 + 3 + 4 + 2 and s.steps_since_reset == 5 + 70 + 9 + 4 + 66
r = comm.rank
np.save(os.path.join(out, "coords_%d.npy" % r), st.coords)
np.save(os.path.join(out, "logp_%d.npy" % r), st.log_prob)
np.save(os.path.join(out, "chain_%d.npy" % r), s.get_chain())
np.save(os.path.join(out, "lnp_%d.npy" % r), s.get_log_prob())
blobs = s.get_blobs()
np.save(os.path.join(out, "blob0_%d.npy" % r), np.asarray(blobs[0]))
np.save(os.path.join(out, "blob1_%d.npy" % r), np.asarray(blobs[1]))
np.save(os.path.join(out, "acc_%d.npy" % r), s.acceptance_fraction)
