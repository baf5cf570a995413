"""Kernel k-means on a precomputed kernel matrix (Dhillon, Guan & Kulis, KDD 2004), as the TCAL learner uses it on a few
dozen samples (ital_amd/competitors.py).  Host numpy: there is nothing here to put on a device.

The squared distance of sample i to the centre of cluster j (members M, n_j of them) in the kernel's feature space is
K_ii - 2 sum_{a in M} K_ia / n_j + sum_{a, b in M} K_ab / n_j^2; the first term is the same for every cluster and is left out.
Random initial labels; every round moves each sample to its nearest centre; stops when fewer than `tol` of the samples moved.
"""
import numpy as np


def kernel_kmeans(K, n_clusters, max_iter=50, tol=1e-3, rng=None):
    """Cluster labels (int array of len(K)) of kernel k-means on the symmetric kernel matrix `K`.

    `rng`: a numpy RandomState; None is numpy's global legacy generator (what `np.random.seed` seeds), from which exactly one
    `randint(n_clusters, size=len(K))` is drawn, the initial labels.  ValueError when a cluster runs empty (the initial draw
    may already leave one out): try fewer clusters."""
    K = np.asarray(K, dtype=np.float64)
    m = K.shape[0]
    if rng is None:
        rng = np.random.mtrand._rand
    labels = rng.randint(n_clusters, size=m)
    dist = np.zeros((m, n_clusters))
    for _ in range(max_iter):
        for j in range(n_clusters):
            members = labels == j
            n_j = int(members.sum())
            if n_j == 0:
                raise ValueError("kernel k-means: cluster %d of %d is empty, try fewer clusters" % (j, n_clusters))
            within = np.sum(K[members][:, members]) / (n_j * n_j)
            dist[:, j] = within - 2 * np.sum(K[:, members], axis=1) / n_j
        previous, labels = labels, dist.argmin(axis=1)
        if 1 - float(np.sum(labels == previous)) / m < tol:
            break
    return labels
