"""numpy restatement of the reference's field post-processing, for the tests of the device kernels:
  von_mises        sqrt(frobeniusNormSq(vonMisesExtractor<N>().doubleContract(s)))                       (VonMises.hh)
  eigenvalues / eigen_decomposition   Eigen's SelfAdjointEigenSolver on the unflattened matrix, ascending (SymmetricMatrix.hh)
  vertex_averaged  vertexAveragedField: volume-weighted average of the element corner values per vertex   (FieldPostProcessing.hh:24-47)
Flattened symmetric matrices carry TENSOR shear entries, 2D xx yy xy, 3D xx yy zz yz xz xy (Flattening.hh). Pinned on closed forms by
tests/test_stress_measures_reference.py."""
import numpy as np

_PAIRS = {2: ((0, 0), (1, 1), (0, 1)), 3: ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))}


def dim_of(flat):
    return {3: 2, 6: 3}[np.shape(flat)[-1]]


def unflatten(flat):
    flat = np.asarray(flat, dtype=np.float64)
    N = dim_of(flat)
    A = np.empty(flat.shape[:-1] + (N, N))
    for k, (i, j) in enumerate(_PAIRS[N]):
        A[..., i, j] = A[..., j, i] = flat[..., k]
    return A


def flatten(A):
    A = np.asarray(A, dtype=np.float64)
    return np.stack([A[..., i, j] for i, j in _PAIRS[A.shape[-1]]], axis=-1)


def von_mises(flat):
    """3D: sqrt(3/2 dev s : dev s). 2D: the plane-stress value sqrt(s00^2 + s11^2 - s00 s11 + 3 s01^2)."""
    s = np.asarray(flat, dtype=np.float64)
    if dim_of(s) == 2:
        return np.sqrt(s[..., 0] ** 2 + s[..., 1] ** 2 - s[..., 0] * s[..., 1] + 3.0 * s[..., 2] ** 2)
    A = unflatten(s)
    dev = A - (np.trace(A, axis1=-2, axis2=-1) / 3.0)[..., None, None] * np.eye(3)
    return np.sqrt(1.5 * np.einsum("...ij,...ij->...", dev, dev))


def eigenvalues(flat):
    return np.linalg.eigvalsh(unflatten(flat))


def eigen_decomposition(flat):
    """(eigenvalues ascending [..., N], eigenvectors in columns [..., N, N])"""
    return np.linalg.eigh(unflatten(flat))


def vertex_averaged(corner_nodes, volumes, field, n_vert):
    """corner_nodes: [nElem, N+1] vertex of every element corner; field: [nElem, 1 | N+1, ...]. Elements in ascending order, as the
    reference's loop (and the device's gather list) visits them."""
    corner_nodes, volumes, field = np.asarray(corner_nodes), np.asarray(volumes, dtype=np.float64), np.asarray(field, dtype=np.float64)
    nE, nc = corner_nodes.shape
    f = np.broadcast_to(field, (nE, nc) + field.shape[2:])
    acc = np.zeros((n_vert,) + field.shape[2:])
    vol = np.zeros(n_vert)
    # np.add.at adds one entry after the other in index order: element by element, like the reference's loop
    np.add.at(acc, corner_nodes.reshape(-1), (volumes.reshape(nE, 1, *([1] * (f.ndim - 2))) * f).reshape((nE * nc,) + field.shape[2:]))
    np.add.at(vol, corner_nodes.reshape(-1), np.repeat(volumes, nc))
    return acc / vol.reshape((n_vert,) + (1,) * (acc.ndim - 1))
