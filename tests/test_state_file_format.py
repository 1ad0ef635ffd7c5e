"""The format of `prefix.<n>.state.npz` with every device product and the bounds ring on (no GPU):
the exact key set, and dtype and shape of every key a product or the ring owns.  A state file of
one version of the sampler resumes under another only while these hold."""
import weakref

import numpy as np

from cobaya_amd.marginals import slab_size
from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import MCMCHip
from tests.autocorr_ref import AcOracleEngine
from tests.test_host_logic import QUICK
from tests.test_marginals_host import MargOracleEngine


class BothEngine(MargOracleEngine, AcOracleEngine):
    """The oracle-backed engine double with the marginal and the autocorrelation methods."""


class OnDouble(MCMCHip):
    _engine_factory = staticmethod(BothEngine)


# what the engine double's get_full_state() and the sampler's own books put into the file
ENGINE_KEYS = {"x", "y", "logpost", "logprior", "loglike", "weight", "prior_rej", "burn_left", "n_accept", "step"}
SAMPLER_KEYS = {"geometry", "acc_n", "acc_gs", "acc_S", "proposal_cov", "shift", "iv_n", "iv_gs", "iv_S", "iv0",
                "book", "fbook", "progress"}


def test_key_set_dtypes_and_shapes_of_the_state_file(tmp_path):
    W, d, lags, bins, bins2d, slots = 128, 2, 3, 16, 4, 16
    p = str(tmp_path / "c")
    s = OnDouble({"seed": 21, "n_walkers": W, "group_size": 64, "steps_per_launch": 40, "max_samples": 60000,
                  "Rminus1_stop": 0.0, "learn_every": "20d", "snapshot_every": 40, "bounds_snapshots": slots,
                  "marginals": {"params": "all", "pairs": [["b", "a"]], "bins": bins, "bins2d": bins2d},
                  "autocorr": {"params": ["b", "a"], "lags": lags}}, ProblemSpec.from_info(QUICK), output=p)
    s.run()
    assert len(s.progress) >= 3 and s._iv0 > 0      # checkpoints were processed, the window dropped intervals
    z = np.load(p + ".1.state.npz", allow_pickle=False)
    n_iv = len(z["iv_n"])
    assert n_iv == len(s._intervals) >= 2
    held = int(np.count_nonzero(z["bslots"] >= 0))
    assert held > 0
    n_counters = slab_size(2, bins, 1, bins2d)
    U = np.dtype("<U1")      # (the names are single letters)
    owned = {
        "marg_params": (U, (2,)), "marg_pairs": (U, (1, 2)), "marg_bins": (np.int64, (2,)),
        "marg_range_names": (U, (2,)), "marg_ranges": (np.float64, (2, 2)),
        "marg_iv": (np.uint64, (n_iv, n_counters)), "marg_open": (np.uint64, (n_counters,)),
        "marg_open_n": (np.int64, ()),
        "ac_params": (U, (2,)), "ac_geometry": (np.int64, (2,)),
        "ac_iv": (np.float64, (n_iv, 3, lags + 1, 2)), "ac_iv_pairs": (np.int64, (n_iv, lags + 1)),
        "ac_open": (np.float64, (3, lags + 1, 2)), "ac_open_pairs": (np.int64, (lags + 1,)),
        "bring": (np.float64, (held, W, d)), "bslots": (np.int64, (slots,)), "bbook": (np.int64, (2,)),
    }
    assert set(z.files) == ENGINE_KEYS | SAMPLER_KEYS | set(owned)
    for k, (dtype, shape) in owned.items():
        assert (z[k].dtype, z[k].shape) == (np.dtype(dtype), shape), (k, z[k].dtype, z[k].shape)
    # the contents that say how to read the rest
    assert z["marg_params"].tolist() == ["a", "b"] and z["marg_pairs"].tolist() == [["b", "a"]]
    assert z["marg_bins"].tolist() == [bins, bins2d] and z["marg_range_names"].tolist() == ["a", "b"]
    assert z["ac_params"].tolist() == ["b", "a"] and z["ac_geometry"].tolist() == [lags, 40]
    assert z["bbook"].tolist() == [s._bounds.stride, s._bounds.n_taken] and z["bslots"].tolist() == s._bounds.slots
    # nothing the sampler holds refers back to it: an engine that nobody closed is freed with the
    # sampler's last reference and does not wait for the cycle collector
    engine = weakref.ref(s.engine)
    del s
    assert engine() is None
