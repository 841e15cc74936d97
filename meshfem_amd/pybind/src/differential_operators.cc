// `differential_operators`: the operators of a FEM mesh as sparse_matrices.TripletMatrix objects, with the function names, argument names
// and defaults of the reference's extension module of that name:
//   laplacian(mesh, forceP1 = False, upperTriOnly = False)          mass(mesh, lumped = False, forceP1 = False, upperTriOnly = False)
//   mass_elasticity(mesh, lumped = False, forceP1 = False, upperTriOnly = False)
//   gradient(mesh, scalarField)                                     divergence(mesh, vectorField)
// Every call assembles on the device through the C++ facade (include/MeshFEMHip/DifferentialOperators.hh): forceP1 on a quadratic mesh is
// the forced-degree-1 view of the same context, mass_elasticity the one-value-per-block operator MFH_OP_MASS_VECTOR. With
// upperTriOnly = False the upper triangle is reflected (TripletMatrix.reflectUpperTriangle), as the reference does.
// The functions take a mesh and keep nothing between calls, like the reference's: EVERY call (gradient and divergence too) builds a fresh
// context and mesh on the device and drops them on return. That is the price of the compatible surface; a caller that applies several
// operators to one mesh keeps a context instead (meshfem_amd.scalar_operators with ctx=, or the facade header on a Simulator).
// `bilaplacian` is NOT provided: it is the sparse-sparse product L diag(1 / m) L returned as a matrix, and a sparse-sparse product has
// no device counterpart in this library (docs/design/08_out_of_scope.md).
#include "common.hh"

#include "../../../include/MeshFEMHip/DifferentialOperators.hh"

namespace {

using MeshFEMHip::check;

// a device context holding the mesh of a `mesh.FEMMesh`
struct MeshContext {
    MeshFEMHip::Context owner;
    size_t N = 0, degree = 0;
    int64_t nElem = 0, nNode = 0;
    explicit MeshContext(const py::object &mesh, int device = 0) : owner(device) {
        const ArrD V = mesh.attr("vertices")().cast<ArrD>();
        const ArrI F = mesh.attr("elements")().cast<ArrI>();
        degree = mesh.attr("degree").cast<size_t>();
        N = mesh.attr("embeddingDimension").cast<size_t>();
        if (V.ndim() != 2 || F.ndim() != 2 || (size_t)V.shape(1) != N || (size_t)F.shape(1) != N + 1)
            throw std::runtime_error("only tet meshes in 3D and triangle meshes in 2D are on the GPU path");
        std::vector<int32_t> f((size_t)F.size());
        for (py::ssize_t k = 0; k < F.size(); ++k) f[(size_t)k] = (int32_t)F.data()[k];
        check(get(), mfh_mesh_build(get(), (int32_t)N, (int32_t)degree, (int64_t)F.shape(0), (int64_t)V.shape(0), f.data(), V.data()));
        check(get(), mfh_mesh_sizes(get(), &nElem, &nNode, nullptr, nullptr, nullptr, nullptr, nullptr));
    }
    mfh_ctx *get() const { return owner.get(); }
};

// facade triplets -> sparse_matrices.TripletMatrix (the class lives in that module)
py::object toTripletMatrix(const MeshFEMHip::TripletMatrix &T, bool lumped, bool upperTriOnly) {
    py::module sm = py::module::import("sparse_matrices");
    py::object A = sm.attr("TripletMatrix")(T.m, T.n);
    py::object addNZ = A.attr("addNZ");
    for (const auto &t : T.nz) addNZ(t.i, t.j, t.v);
    if (!lumped) A.attr("symmetry_mode") = sm.attr("SymmetryMode").attr("UPPER_TRIANGLE");    // (a lumped matrix is diagonal: MassMatrix.hh:123-124)
    if (!upperTriOnly) A.attr("reflectUpperTriangle")();
    return A;
}

py::object construct(const py::object &mesh, int32_t op, bool lumped, bool forceP1, bool upperTriOnly) {
    MeshContext mc(mesh);
    const MeshFEMHip::TripletMatrix T = forceP1 ? MeshFEMHip::detail::operatorTriplets<1>(mc.get(), op, lumped)
                                                : MeshFEMHip::detail::operatorTriplets<MeshFEMHip::detail::kMeshDegree>(mc.get(), op, lumped);
    return toTripletMatrix(T, lumped, upperTriOnly);
}

}   // namespace

PYBIND11_MODULE(differential_operators, m) {
    m.doc() = "Differential operators provided by a FEM discretization (MI355X path: assembled on the device through libmeshfem_hip). "
              "Every call builds its own device context and mesh and drops them on return; keep a meshfem_amd Context "
              "(meshfem_amd.scalar_operators, ctx=) to apply several operators to one mesh. "
              "bilaplacian is not provided: a sparse-sparse product has no device counterpart in this library.";
    py::module::import("mesh");
    py::module::import("sparse_matrices");

    m.def("laplacian", [](const py::object &mesh, bool forceP1, bool upperTriOnly) { return construct(mesh, MFH_OP_LAPLACIAN, false, forceP1, upperTriOnly); },
          py::arg("mesh"), py::arg("forceP1") = false, py::arg("upperTriOnly") = false);
    m.def("mass", [](const py::object &mesh, bool lumped, bool forceP1, bool upperTriOnly) { return construct(mesh, MFH_OP_MASS, lumped, forceP1, upperTriOnly); },
          py::arg("mesh"), py::arg("lumped") = false, py::arg("forceP1") = false, py::arg("upperTriOnly") = false);
    m.def("mass_elasticity", [](const py::object &mesh, bool lumped, bool forceP1, bool upperTriOnly) { return construct(mesh, MFH_OP_MASS_VECTOR, lumped, forceP1, upperTriOnly); },
          py::arg("mesh"), py::arg("lumped") = false, py::arg("forceP1") = false, py::arg("upperTriOnly") = false, "Mass matrix for vector-valued shape functions");
    m.def("gradient", [](const py::object &mesh, const ArrD &scalarField) {
        MeshContext mc(mesh);
        if (mc.degree > 1) throw std::runtime_error("Interpolant type bindings unimplemented...");            // as the reference
        if (scalarField.ndim() != 1 || scalarField.shape(0) != mc.nNode) throw std::runtime_error("Incorrect scalar field size");
        ArrD g = make2d((size_t)mc.nElem, mc.N);
        check(mc.get(), mfh_average_gradient(mc.get(), scalarField.data(), g.mutable_data()));
        return g;
    }, py::arg("mesh"), py::arg("scalarField"));
    m.def("divergence", [](const py::object &mesh, const ArrD &vectorField) {
        MeshContext mc(mesh);
        if (mc.degree > 1) throw std::runtime_error("Interpolant type bindings unimplemented...");
        if (vectorField.ndim() != 2 || vectorField.shape(0) != mc.nElem || (size_t)vectorField.shape(1) != mc.N) throw std::runtime_error("Incorrect vector field size");
        ArrD out((py::ssize_t)mc.nNode);
        check(mc.get(), mfh_divergence(mc.get(), vectorField.data(), out.mutable_data()));
        return out;
    }, py::arg("mesh"), py::arg("vectorField"));
}
