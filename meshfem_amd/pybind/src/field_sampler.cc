// `field_sampler`: point queries on a mesh, with the class name, method names, argument names and defaults of the reference's extension
// module of that name:
//   FieldSampler(mesh)   on a mesh.Mesh            FieldSampler(V, F)   a raw mesh: a degree-1 context of its own
//   closestElementAndPoint(P) -> (I, C)            closestElementAndBaryCoords(P) -> (I, B)
//   closestNodeAndSqDist(P) -> (NI, sqDist)        contains(P, eps = 1e-10)            sample(P, fieldValues)
// Every sampler builds a device context OF ITS OWN with the mesh (C ABI: mfh_locate, mfh_sample_field, mfh_closest_node) and keeps it, with its
// cell grids, until it is dropped. FieldSampler(mesh) does not share the context the mesh.Mesh object holds: it reads vertices(), elements() and
// degree from it and builds the mesh again, a second copy on the device. Per-node fields line up with mesh.nodes() because the node numbering is a
// function of (vertices, elements, degree) alone (the same library code numbers both). What differs from the reference: a uniform cell grid instead of the AABB tree; a point shared by several elements goes
// to the one with the LOWEST index; triangle meshes embedded in 3D are refused (the contexts of this library are planar);
// closestNodeAndSqDist on a raw mesh throws "Unsupported for raw meshes" as the reference does.
#include "common.hh"

#include <memory>

namespace {

using MeshFEMHip::check;

struct Sampler {
    MeshFEMHip::Context owner;
    bool raw = false;
    size_t N = 0;
    int64_t nVert = 0, nElem = 0, nNode = 0;

    Sampler(const ArrD &V, const ArrI &F, size_t degree, bool isRaw, int device = 0) : owner(device), raw(isRaw) {
        if (V.ndim() != 2 || F.ndim() != 2) throw std::runtime_error("V and F must be matrices");
        N = (size_t)V.shape(1);
        if ((size_t)F.shape(1) == 3 && N == 3)
            throw std::runtime_error("FieldSampler: triangle meshes embedded in 3D are not supported on the GPU path (its contexts are planar); pass 2D vertex positions");
        if ((N != 2 && N != 3) || (size_t)F.shape(1) != N + 1)
            throw std::runtime_error("only tet meshes in 3D and triangle meshes in 2D are on the GPU path");
        std::vector<int32_t> f((size_t)F.size());
        for (py::ssize_t k = 0; k < F.size(); ++k) f[(size_t)k] = (int32_t)F.data()[k];
        check(owner.get(), mfh_mesh_build(owner.get(), (int32_t)N, (int32_t)degree, (int64_t)F.shape(0), (int64_t)V.shape(0), f.data(), V.data()));
        check(owner.get(), mfh_mesh_sizes(owner.get(), &nElem, &nNode, &nVert, nullptr, nullptr, nullptr, nullptr));
    }
    mfh_ctx *ctx() const { return owner.get(); }
    py::ssize_t points(const ArrD &P) const {
        if (P.ndim() != 2 || (size_t)P.shape(1) != N) throw std::runtime_error("P must hold one query point per row (nP x " + std::to_string(N) + ")");
        return P.shape(0);
    }
};

py::array_t<int32_t> makeInts(py::ssize_t n) { return py::array_t<int32_t>(n); }

}   // namespace

PYBIND11_MODULE(field_sampler, m) {
    m.doc() = "Point location and field evaluation on a mesh (MI355X path: a uniform cell grid and the query kernels of libmeshfem_hip). "
              "A point shared by several elements is assigned to the one with the lowest index; triangle meshes embedded in 3D are refused. "
              "FieldSampler(mesh) builds a device context of its own from mesh.vertices(), mesh.elements() and mesh.degree (a second copy of the "
              "mesh on the device); the node numbering is the same as the mesh object's.";

    py::class_<Sampler>(m, "FieldSampler")
        .def(py::init([](const py::object &mesh) {
                 const ArrD V = mesh.attr("vertices")().cast<ArrD>();
                 const ArrI F = mesh.attr("elements")().cast<ArrI>();
                 const size_t N = mesh.attr("embeddingDimension").cast<size_t>();
                 if (V.ndim() == 2 && (size_t)V.shape(1) != N) throw std::runtime_error("mesh: vertex positions do not match the embedding dimension");
                 return new Sampler(V, F, mesh.attr("degree").cast<size_t>(), false);
             }), py::arg("mesh"))
        .def(py::init([](const ArrD &V, const ArrI &F) { return new Sampler(V, F, 1, true); }), py::arg("V"), py::arg("F"))
        .def("closestElementAndPoint", [](const Sampler &s, const ArrD &P) {
                 const py::ssize_t n = s.points(P);
                 py::array_t<int32_t> I = makeInts(n);
                 ArrD C = make2d((size_t)n, s.N);
                 check(s.ctx(), mfh_locate(s.ctx(), n, P.data(), I.mutable_data(), nullptr, C.mutable_data(), nullptr, 0));
                 return py::make_tuple(I, C);
             }, py::arg("P"))
        .def("closestElementAndBaryCoords", [](const Sampler &s, const ArrD &P) {
                 const py::ssize_t n = s.points(P);
                 py::array_t<int32_t> I = makeInts(n);
                 ArrD B = make2d((size_t)n, s.N + 1);
                 check(s.ctx(), mfh_locate(s.ctx(), n, P.data(), I.mutable_data(), B.mutable_data(), nullptr, nullptr, 0));
                 return py::make_tuple(I, B);
             }, py::arg("P"))
        .def("closestNodeAndSqDist", [](const Sampler &s, const ArrD &P) {
                 if (s.raw) throw std::runtime_error("Unsupported for raw meshes");
                 const py::ssize_t n = s.points(P);
                 py::array_t<int32_t> NI = makeInts(n);
                 ArrD sq((py::ssize_t)n);
                 check(s.ctx(), mfh_closest_node(s.ctx(), n, P.data(), NI.mutable_data(), sq.mutable_data(), 0));
                 return py::make_tuple(NI, sq);
             }, py::arg("P"))
        .def("contains", [](const Sampler &s, const ArrD &P, double eps) {
                 const py::ssize_t n = s.points(P);
                 std::vector<double> sq((size_t)n);
                 check(s.ctx(), mfh_locate(s.ctx(), n, P.data(), nullptr, nullptr, nullptr, sq.data(), 0));
                 py::array_t<bool> out(n);
                 for (py::ssize_t i = 0; i < n; ++i) out.mutable_data()[i] = sq[(size_t)i] <= eps * eps;
                 return out;
             }, py::arg("P"), py::arg("eps") = 1e-10)
        .def("sample", [](const Sampler &s, const ArrD &P, const ArrD &fieldValues) {
                 const py::ssize_t n = s.points(P);
                 if (fieldValues.ndim() < 1 || fieldValues.ndim() > 2) throw std::runtime_error("Invalid fieldValues size");
                 const int64_t rows = fieldValues.shape(0);
                 int32_t kind;
                 if (rows == s.nVert) kind = MFH_FIELD_PER_VERTEX;               // the reference's order: vertices, elements, nodes
                 else if (rows == s.nElem) kind = MFH_FIELD_PER_ELEMENT;
                 else if (rows == s.nNode) kind = MFH_FIELD_PER_NODE;
                 else throw std::runtime_error("Invalid fieldValues size");
                 const py::ssize_t nComp = fieldValues.ndim() == 2 ? fieldValues.shape(1) : 1;
                 if (nComp < 1) throw std::runtime_error("Invalid fieldValues size");
                 ArrD out = fieldValues.ndim() == 2 ? make2d((size_t)n, (size_t)nComp) : ArrD(n);
                 check(s.ctx(), mfh_sample_field(s.ctx(), n, P.data(), kind, fieldValues.data(), (int32_t)nComp, out.mutable_data(), 0));
                 return out;
             }, py::arg("P"), py::arg("fieldValues"));
}
