"""Randomized parity soak of Frame::ComputeBoW on the device (orbx_vocab.hip: breadth-first descent, register / LDS bitonic sorts, sequential L1 norm)
against the CPU oracle's DBoW2 restatement: random vocabularies (k, L, stop words), feature counts on both sides of every sort-size and
chunk boundary, levelsup 0..L.  Half of the vocabularies are level-by-level full trees (synth.vocab_tree), half are numbered and shaped
as DBoW2 builds them (synth.vocab_tree_dbow2: k up to 20, ragged sibling groups, leaves at every level, tied siblings).
python tools/soak_vocab.py [seconds] [seed]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as ge
from tools import synth
from oracle import oracle_py as O
pkg = ge.load_pkg()
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 2024))
t0 = time.time(); trials = feats = 0
edge = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 2000, 2047, 2048, 2049, 4095, 4096, 4097, 6000]
while time.time() - t0 < budget:
    k = int(rng.integers(2, 13)); L = int(rng.integers(1, 6))
    while k ** L > 200000: L -= 1
    n = int(rng.choice(edge)) if rng.random() < 0.5 else int(rng.integers(1, 3000))
    data = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if rng.random() < 0.3 and n > 4:          # duplicates: several features per word
        data[rng.integers(0, n, n // 3)] = data[rng.integers(0, n, n // 3)]
    stop = float(rng.choice([0.0, 0.05, 0.3]))
    if trials % 2:                            # DBoW2's own node order and shape
        k = int(rng.integers(2, 21)); L = int(rng.integers(1, 11))
        par, leaf, nd, w = synth.vocab_tree_dbow2(int(rng.integers(0, 1 << 30)), k, L, n_feat=int(rng.integers(k + 1, 6000)), stop_frac=stop,
                                                  single_frac=float(rng.choice([0.0, 0.2, 0.5])), dup910_frac=float(rng.choice([0.0, 0.5, 1.0])))
        if rng.random() < 0.7:                # features near the leaves, else the random ones above
            data = synth.vocab_features(int(rng.integers(0, 1 << 30)), leaf, nd, n, 0.04)
    else:
        par, leaf, nd, w = synth.vocab_tree(int(rng.integers(0, 1 << 30)), k, L, stop_frac=stop, data=data)
    V = pkg.ORBVocabulary(k, L, par, leaf, nd, w); OV = O.Vocabulary(k, L, par, leaf, nd, w)
    for levelsup in {0, int(rng.integers(0, L + 2)), 4}:
        got = V.transform(data, levelsup); exp = OV.transform(data, levelsup)
        for key in exp:
            assert got[key].dtype == exp[key].dtype and got[key].shape == exp[key].shape and got[key].tobytes() == exp[key].tobytes(), (k, L, n, levelsup, key)
    trials += 1; feats += n
print("vocab soak done: %d vocabularies / feature sets (%d features), BowVector and FeatureVector byte-equal to the oracle" % (trials, feats))
