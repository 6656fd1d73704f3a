"""Synthetic place-recognition scenes for the KeyFrameDatabase tests and tools/bench_kfdb.py.

Independent random BowVectors make a place-recognition query trivial (one keyframe passes the 0.8 gate, no neighbour ever wins, no
stale score is read), so keyframes are drawn from PLACES: a place owns `base` words; a view of it (a keyframe or a query) keeps a random
`keep` share of them plus `extra` words from anywhere.  Values span several decades and are L1-normalised by a sequential sum, as
BowVector::normalize does.  Covisibility lists hold keyframes of the same place plus a few random ones."""
import numpy as np


def view(rng, base_words, nwords, keep=0.6, extra=240, decades=3.0):
    """one BowVector seen at a place: (uint32 ids ascending, float64 values with L1 norm 1)"""
    kept = base_words[rng.random(len(base_words)) < keep]
    ids = np.unique(np.concatenate([kept, rng.integers(0, nwords, extra)])).astype(np.uint32)
    raw = 10.0 ** rng.uniform(-decades, 0.0, len(ids))
    norm = 0.0
    for v in raw:
        norm += float(v)
    return ids, (raw / norm).astype(np.float64)


class Scene:
    def __init__(self, seed, places=25, per_place=8, nwords=100000, base=600, keep=0.6, extra=240, same=5, other=3):
        self.rng = np.random.default_rng(seed)
        self.nwords, self.keep, self.extra = nwords, keep, extra
        self.bases = [np.sort(self.rng.choice(nwords, base, replace=False)) for _ in range(places)]
        self.place_of = [p for p in range(places) for _ in range(per_place)]
        self.keyframes = [view(self.rng, self.bases[p], nwords, keep, extra) for p in self.place_of]
        n = len(self.keyframes)
        self.neighbours = []
        for i in range(n):
            first = self.place_of[i] * per_place
            mates = [j for j in range(first, first + per_place) if j != i]
            pick = list(self.rng.permutation(mates)[:same]) + list(self.rng.integers(0, n, other))
            self.neighbours.append([int(j) for j in self.rng.permutation(pick)][:10])

    def query(self, place=None, second=None, share=0.5):
        """a view of `place` (random when None); with `second`, a mixture of two places"""
        p = int(self.rng.integers(0, len(self.bases))) if place is None else place
        words = self.bases[p]
        if second is not None:
            a = words[self.rng.random(len(words)) < share]
            b = self.bases[second][self.rng.random(len(self.bases[second])) < 1.0 - share]
            words = np.unique(np.concatenate([a, b]))
        return view(self.rng, words, self.nwords, self.keep, self.extra)
