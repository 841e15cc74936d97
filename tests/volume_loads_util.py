"""FP64 restatement of the volume loads (mfh_body_force_load, mfh_stress_field_load; docs/design/04_14_volume_loads.md), written from the
mathematics and independently of the library's shape tables: the shape functions are polynomials in the barycentric coordinates
(vertex nodes first, then one node per edge in the order of the oracle's EDGE_START / EDGE_END), their integrals come from the exact simplex
formula  int l^a = d! a! / (|a| + d)! vol,  grad l from the vertex coordinates by inverting the affine map. Materials are the D matrices of
element_integrals_util.material. Loads are per-DoF vectors [nDoF, dim], summed in element order, fields as the library takes them: flattened symmetric tensors with TENSOR shear entries."""
import math

import numpy as np

from oracle import meshfem_oracle as O


def shape_polynomials(dim, deg):
    """every shape function as a list of (coefficient, exponents of l_0 .. l_dim)"""
    nv = dim + 1
    unit = lambda *ks: tuple(sum(1 for k in ks if k == j) for j in range(nv))
    if deg == 1:
        return [[(1.0, unit(i))] for i in range(nv)]
    polys = [[(2.0, unit(i, i)), (-1.0, unit(i))] for i in range(nv)]                      # l_i (2 l_i - 1)
    polys += [[(4.0, unit(O.EDGE_START[e], O.EDGE_END[e]))] for e in range(O.num_edges(dim))]   # 4 l_s l_t
    return polys


def monomial_integral(dim, expo):
    """int over the unit-volume simplex of prod l_k^expo_k"""
    return math.factorial(dim) * math.prod(math.factorial(a) for a in expo) / math.factorial(sum(expo) + dim)


def poly_mul(p, q):
    return [(a * b, tuple(x + y for x, y in zip(ea, eb))) for a, ea in p for b, eb in q]


def poly_integral(dim, p):
    return sum(c * monomial_integral(dim, e) for c, e in p)


def weights(dim, deg):
    """w_i = int phi_i / vol"""
    return np.array([poly_integral(dim, p) for p in shape_polynomials(dim, deg)])


def mass_coefficients(dim, deg):
    """m_ij = int phi_i phi_j / vol"""
    P = shape_polynomials(dim, deg)
    return np.array([[poly_integral(dim, poly_mul(p, q)) for q in P] for p in P])


def poly_gradient_coefficients(dim, deg):
    """G[i, k] = int (d phi_i / d l_k) / vol: int grad phi_i = vol sum_k G[i, k] grad l_k"""
    nv = dim + 1
    G = np.zeros((len(shape_polynomials(dim, deg)), nv))
    for i, p in enumerate(shape_polynomials(dim, deg)):
        for c, e in p:
            for k in range(nv):
                if e[k]:
                    d = list(e)
                    d[k] -= 1
                    G[i, k] += c * e[k] * monomial_integral(dim, d)
    return G


def geometry(verts, corners):
    """(vol [nE], grad l [nE, nv, dim]) of the simplices with the given corner vertices: l(x) = A^-1 (1, x) with A = [[1 .. 1], [p_0 .. p_d]]"""
    P = np.asarray(verts, dtype=np.float64)[np.asarray(corners)]          # [nE, nv, dim]
    nE, nv, dim = P.shape
    A = np.concatenate([np.ones((nE, 1, nv)), np.swapaxes(P, 1, 2)], axis=1)
    vol = np.abs(np.linalg.det(A)) / math.factorial(dim)
    return vol, np.linalg.inv(A)[:, :, 1:]


class Mesh:
    def __init__(self, dim, deg, elem_nodes, node_pos, dof=None, n_dof=None):
        self.dim, self.deg = dim, deg
        self.en = np.asarray(elem_nodes, dtype=np.int64)
        self.vol, self.gl = geometry(node_pos, self.en[:, :dim + 1])
        n_node = len(node_pos)
        self.dof = np.arange(n_node) if dof is None else np.asarray(dof, dtype=np.int64)
        self.n_dof = n_node if n_dof is None else int(n_dof)

    def scatter(self, fe):
        """per-(element, local node) vectors [nE, npe, dim] -> per-DoF, added in element order"""
        idx = self.dof[self.en].ravel()                  # (np.bincount adds its weights one after the other, in this order)
        return np.stack([np.bincount(idx, weights=fe[:, :, c].ravel(), minlength=self.n_dof) for c in range(self.dim)], axis=1)

    def unflatten(self, s):
        F = np.array([[O.flatten_indices(self.dim, i, j) for j in range(self.dim)] for i in range(self.dim)])
        return np.asarray(s, dtype=np.float64)[..., F]

    def stress_of_strain(self, D, eps):
        """C_e : eps_e for flattened strains [nE, fl]: D times the shear-doubled strain"""
        D = np.asarray(D, dtype=np.float64)
        dbl = np.where(np.arange(D.shape[-1]) < self.dim, 1.0, 2.0)
        return np.einsum("erc,ec->er", np.broadcast_to(D, (len(self.en),) + D.shape[-2:]), np.asarray(eps) * dbl)

    def stress_field_load(self, sigma):
        """f_i = sum_e sigma_e . int_e grad phi_i"""
        gint = self.vol[:, None, None] * np.einsum("ik,ekb->eib", poly_gradient_coefficients(self.dim, self.deg), self.gl)
        return self.scatter(np.einsum("ecb,eib->eic", self.unflatten(sigma), gint))

    def body_force_load(self, b, density=None):
        """f_i = sum_e rho_e int_e phi_i b; b: (dim,), (nE, dim) or (nNode, dim)"""
        b = np.asarray(b, dtype=np.float64)
        rv = self.vol if density is None else np.asarray(density) * self.vol
        if b.shape == (self.dim,) or b.shape == (len(self.en), self.dim):
            be = np.broadcast_to(b, (len(self.en), self.dim))
            return self.scatter(rv[:, None, None] * weights(self.dim, self.deg)[None, :, None] * be[:, None, :])
        return self.scatter(rv[:, None, None] * np.matmul(mass_coefficients(self.dim, self.deg), b[self.en]))
