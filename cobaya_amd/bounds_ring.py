"""The host side of the ring behind R-1 of the confidence bounds (mcmc.py:918-1002): which ensemble
snapshot each of the engine's slots holds (mcmc_hip_bounds_*), and how the ring is saved and restored.
Not an interval product (marginals.py): its life cycle is take / window / save / load."""
from __future__ import annotations

import os

import numpy as np


class BoundsRing:
    """`slots`: slot -> index of the moment snapshot it holds (-1: free); `stride`: of the thinned
    record; `n_taken`: moment snapshots seen so far.  `shape`: (walkers, d) of a snapshot; `files`:
    the paths of this process' two sidecar files (None: the run has no output)."""

    SAVE_BYTES = 1 << 26   # snapshots kept in the state file; a larger ring goes to the sidecar
    FILES = ("bounds.npy", "bounds_tags.npy")   # the sidecar: the snapshots, the snapshot of each slot

    def __init__(self, engine, n_slots=0, shape=None, files=None):
        self.engine, self.shape, self.files = engine, shape, files
        self.slots, self.stride, self.n_taken = [-1] * n_slots, 1, 0

    @classmethod
    def from_option(cls, n, engine, group_size, fail, shape, files):
        """`bounds_snapshots` ensemble snapshots on the device (mcmc_hip_bounds_configure)."""
        if int(n or 0) < 0:
            fail("bounds_snapshots must be >= 0, got %r", n)
        n = int(n or 0) if hasattr(engine, "bounds_configure") else 0
        if n:
            n = min(n, getattr(engine, "BOUNDS_MAX_SLOTS", 64), 16384 // group_size)
            engine.bounds_configure(n)
        return cls(engine, n, shape, files)

    def take(self):
        """Called with every moment snapshot (index i): the ring keeps every `stride`-th one of
        the later half of the run -- the window of mcmc.py:787-790, `use_first = n / 2`.  A slot
        is free once its snapshot has left that window; when none is, the record is thinned
        (stride doubled, every other kept snapshot dropped)."""
        i = self.n_taken
        self.n_taken += 1
        if not self.slots or i % self.stride:
            return
        start = (i + 1) / 2.0
        free = [k for k, j in enumerate(self.slots) if j < start]
        if not free:
            self.stride *= 2
            self.slots = [j if j % self.stride == 0 else -1 for j in self.slots]
            if i % self.stride:
                return
            free = [k for k, j in enumerate(self.slots) if j < 0]
        k = min(free, key=lambda k_: self.slots[k_])
        self.slots[k] = i
        self.engine.bounds_snapshot(k)

    def window(self):
        """The sorted (snapshot index, slot) pairs of the later half of the run."""
        start = self.n_taken / 2.0
        return sorted((j, k) for k, j in enumerate(self.slots) if j >= start)

    # -- the state file and the sidecar
    def save(self):
        """-> arrays for the state file: the books always, the snapshots while they are small (a
        resumed run then forms the same Rminus1_cl); a large ring is written to the sidecar."""
        out = {}
        held = [k for k, j in enumerate(self.slots) if j >= 0]
        if held and 8 * len(held) * self.shape[0] * self.shape[1] <= self.SAVE_BYTES:
            out["bring"] = np.array([self.engine.bounds_get_slot(k) for k in held])
        elif held:
            self._save_sidecar()
        out["bslots"] = np.array(self.slots, dtype=np.int64)
        out["bbook"] = np.array([self.stride, self.n_taken], dtype=np.int64)
        return out

    def load(self, z, log):
        """Restore from the state file `z`: the snapshots are in it, or vouched for by the sidecar,
        or the slots restart empty."""
        if "bbook" not in z or not self.slots:
            return
        self.stride, self.n_taken = (int(v) for v in z["bbook"])
        saved = [int(j) for j in z["bslots"]]
        held = [k for k, j in enumerate(saved) if j >= 0]
        if "bring" in z and len(saved) == len(self.slots):
            self.slots = saved
            for k, x in zip(held, z["bring"]):
                self.engine.bounds_set_slot(k, x)
        elif held and len(saved) == len(self.slots):
            self.slots, n_back = self._load_sidecar(saved)
            if n_back < len(held):
                log.info("%d of the %d snapshots behind R-1 of the bounds were not found "
                         "beside the state file: those slots restart empty.",
                         len(held) - n_back, len(held))
        elif held:
            log.info("bounds_snapshots changed since the checkpoint: the ring behind R-1 "
                     "of the bounds restarts empty.")

    def _sidecar(self, mode):
        """-> (the snapshots, memory-mapped; the tags) where both files are there, readable and of
        this ring's shape; else (None, None)."""
        try:
            mm, tags = np.load(self.files[0], mmap_mode=mode), np.load(self.files[1])
        except Exception:
            return None, None
        ok = mm.shape == (len(self.slots), *self.shape) and tags.shape == (len(self.slots),)
        return (mm, tags) if ok else (None, None)

    def _save_sidecar(self):
        """A bounds ring too large for the state file (251 MB at BASELINE config 2: 16 slots of
        65 536 x 30 doubles) lives in a sidecar `prefix.<n>.bounds.npy` of fixed shape
        [slots][W][d], written IN PLACE and only where a slot's snapshot changed since the last
        dump; `prefix.<n>.bounds_tags.npy` (replaced atomically, after the data) says which
        snapshot each slot of the file holds.  A resumed run restores exactly the slots whose tag
        equals the state file's book -- after a crash between the two writes a slot is dropped,
        never mixed up -- so Rminus1_cl after a resume is the uninterrupted run's."""
        data_f, tags_f = self.files
        mm, tags = self._sidecar("r+")
        if mm is None:
            mm = np.lib.format.open_memmap(data_f, mode="w+", dtype=np.float64,
                                           shape=(len(self.slots), *self.shape))
            tags = np.full(len(self.slots), -1, dtype=np.int64)
        dirty = [k for k, j in enumerate(self.slots) if j >= 0 and tags[k] != j]
        if dirty:   # (the tags of the slots being rewritten are invalid until the data is down)
            tags[dirty] = -1
            np.save(tags_f + ".tmp.npy", tags)
            os.replace(tags_f + ".tmp.npy", tags_f)
            for k in dirty:
                mm[k] = self.engine.bounds_get_slot(k)
            mm.flush()
        tags[:] = self.slots     # (a free slot is -1 in both)
        del mm
        np.save(tags_f + ".tmp.npy", tags)
        os.replace(tags_f + ".tmp.npy", tags_f)

    def _load_sidecar(self, saved):
        """-> the slot books after restoring what the sidecar vouches for (see above), their number."""
        out, n = [-1] * len(saved), 0
        mm, tags = self._sidecar("r")
        for k, j in enumerate(saved if mm is not None else ()):
            if j >= 0 and int(tags[k]) == j:
                self.engine.bounds_set_slot(k, np.array(mm[k]))
                out[k] = j
                n += 1
        return out, n
