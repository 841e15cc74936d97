// C++ drop-in test of explicitTransient / stableTimeStep (include/MeshFEMHip/Dynamics.hh) and lumpedMassHRZ (MassProperties.hh) on a quadratic tet
// Simulator clamped on its face x = min and pulled on its face x = max: writes what two chained calls of explicitTransient (the second started from
// the first's u, v, a) return; tests/test_cpp_explicit.py compares it with the Python layer's on the same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), nSteps, density, output file (f64 dt, lambdaUpper,
// lambdaEst, then m[nDoF][3], u[nDoF][3], v[nDoF][3], a[nDoF][3], probes[nSteps + 1][2], energies[nSteps / 2 + 1][4], the snapshots of every
// second step).
#include <MeshFEMHip/Dynamics.hh>
#include <MeshFEMHip/MassProperties.hh>
#include <cstdio>
#include <cstdlib>

using namespace MeshFEMHip;

int main(int argc, char **argv) {
    const int device = argc > 1 ? atoi(argv[1]) : 0;
    std::vector<std::array<Real, 3>> V = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};      // one tetrahedron: enough to reach the device (or fail to)
    std::vector<std::array<int32_t, 4>> T = {{0, 1, 2, 3}};
    if (argc > 2) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) { printf("cannot open %s\n", argv[2]); return 2; }
        int64_t nv = 0, ne = 0;
        bool ok = fread(&nv, 8, 1, f) == 1 && fread(&ne, 8, 1, f) == 1;
        V.resize((size_t)nv); T.resize((size_t)ne);
        ok = ok && fread(V.data(), sizeof(V[0]), (size_t)nv, f) == (size_t)nv && fread(T.data(), sizeof(T[0]), (size_t)ne, f) == (size_t)ne;
        fclose(f);
        if (!ok) { printf("truncated mesh file\n"); return 2; }
    }
    const int nSteps = argc > 3 ? atoi(argv[3]) : 2;
    const Real density = argc > 4 ? atof(argv[4]) : 1.0;
    try {
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0, 0, 0}, true);
        sim.applyNeumannBox({1.0 - 1e-9, -1e-9, -1e-9}, {1.0 + 1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0.0, 0.0, -1.0}, MFH_NEUMANN_TRACTION, true);
        const mfh_explicit_dt_info lim = stableTimeStep(sim, density);
        const auto mass = lumpedMassHRZ(sim);
        if (!(lim.lambdaUpper >= lim.lambdaEst && lim.lambdaEst > 0 && lim.dtSafe <= lim.dtEst) || mass.size() != sim.numDoFs()) {
            printf("FAILED: the bounds of the stable step\n");
            return 2;
        }
        for (const auto &m : mass)
            if (!(m[0] > 0 && m[0] == m[1] && m[1] == m[2])) { printf("FAILED: a lumped mass is not positive\n"); return 2; }
        ExplicitOptions<Sim::VField> opt;
        opt.density = density;
        opt.rayleighMass = 0.05;
        for (int k = 0; k <= nSteps; ++k) opt.amplitude.push_back(k % 3 == 0 ? 1.0 : 0.5);
        opt.probes = {{sim.numDoFs() - 1, 2}, {sim.numDoFs() / 2, 0}};
        opt.snapshotStride = 2;
        opt.energies = true;
        opt.energyStride = 2;
        // two chained halves through (u0, v0, a0): the second continues the first, and together they are the run of nSteps steps
        const int half = nSteps / 2;
        const std::vector<Real> amp = opt.amplitude;
        opt.amplitude.assign(amp.begin(), amp.begin() + half + 1);
        const auto r1 = explicitTransient(sim, half, 0.0, opt);                   // dt = safety x dtEst
        opt.amplitude.assign(amp.begin() + half, amp.end());
        opt.u0 = r1.u; opt.v0 = r1.v; opt.a0 = r1.a;
        auto r = explicitTransient(sim, nSteps - half, r1.dt, opt);
        if (r1.info.stepsDone != half || r.info.stepsDone != nSteps - half || half % 2 != 0 || r.probes.empty() || r.snapshots.empty() ||
            r1.dt != opt.safety * lim.dtEst || !(r1.info.dtEst > 0)) {
            printf("FAILED: steps of the halves\n");
            return 2;
        }
        r.probes.insert(r.probes.begin(), r1.probes.begin(), r1.probes.end() - 1);
        r.energies.insert(r.energies.begin(), r1.energies.begin(), r1.energies.end() - 1);
        r.snapshots.insert(r.snapshots.begin(), r1.snapshots.begin(), r1.snapshots.end() - 1);
        if (r.u.size() != sim.numDoFs() || r.probes.size() != (size_t)nSteps + 1 || r.snapshots.size() != (size_t)nSteps / 2 + 1 ||
            r.energies.size() != (size_t)nSteps / 2 + 1) {
            printf("FAILED: sizes / steps\n");
            return 2;
        }
        // a step above the stability estimate is refused
        bool refused = false;
        try { (void)explicitTransient(sim, 2, 1.2 * lim.dtEst, opt); } catch (const std::runtime_error &) { refused = true; }
        if (!refused) { printf("FAILED: dt above the estimate was accepted\n"); return 2; }
        if (argc > 5) {
            FILE *f = fopen(argv[5], "wb");
            if (!f) { printf("cannot write %s\n", argv[5]); return 2; }
            const Real head[3] = {r1.dt, lim.lambdaUpper, lim.lambdaEst};
            fwrite(head, sizeof(Real), 3, f);
            const Sim::VField *fields[4] = {&mass, &r.u, &r.v, &r.a};
            for (const Sim::VField *x : fields) fwrite(&(*x)[0][0], sizeof(Real), 3 * x->size(), f);
            for (const auto &p : r.probes) fwrite(p.data(), sizeof(Real), p.size(), f);
            for (const auto &e : r.energies) fwrite(e.data(), sizeof(Real), 4, f);
            for (const auto &s : r.snapshots) fwrite(&s[0][0], sizeof(Real), 3 * s.size(), f);
            fclose(f);
        }
        printf("%d + %d steps at dt %.6g (dtSafe %.6g, dtEst %.6g)\n", half, (int)r.info.stepsDone, r1.dt, lim.dtSafe, lim.dtEst);
        printf("explicit ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
