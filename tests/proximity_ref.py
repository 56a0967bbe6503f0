"""A plain NumPy restatement of the forest proximities (include/sbag.h): leaves from
predict_ref.walk, pair counts by comparing them, moments and randomForest's outlier() from the
counts."""
import numpy as np

import predict_ref as ref


def leaves(trees, subs, X):
    """int32 [N][L]: the node id of the leaf every row reaches in every tree."""
    return np.stack([ref.walk(t, s, X) for t, s in zip(trees, subs)], axis=1).astype(np.int32)


def counts(La, Lb):
    return (La[:, None, :] == Lb[None, :, :]).sum(-1)


def moments(cnt, groups, G):
    out = np.zeros((cnt.shape[0], G, 2), np.uint64)
    for g in range(G):
        c = cnt[:, np.asarray(groups) == g].astype(np.uint64)
        out[:, g, 0] = c.sum(1)
        out[:, g, 1] = (c * c).sum(1)
    return out


def outlier(cnt, trees, labels):
    n = len(labels)
    out = np.zeros(n)
    for c in np.unique(labels):
        own = labels == c
        raw = n / ((cnt[own][:, own].astype(np.float64) ** 2).sum(1) / (float(trees) * float(trees)))
        dev = raw - np.median(raw)
        out[own] = dev / np.median(np.abs(dev))
    return out
