// The bundled block adjusted from intersected start values of its object points: reads the AICON flat files
// <base>.obc/.scale/.ior/.eor/.phc as example_flatfiles does, computes every object point from the image rays that see it
// (ForwardIntersection::intersectAll, one device call for all points; the .obc values are ignored), prints the largest distance of an
// intersected start value from its .obc value, then runs estimateModel() with MatrixInversion::REDUCED.  The orientations are those of
// the .eor file; with --dlt they are first replaced by the DLT's, as example_dlt does (the .obc coordinates as control).
//   usage: example_intersection <base path> [--dlt]
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "aicon_reader.hpp"

using namespace jaicov::host;

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <base path of the .obc/.scale/.ior/.eor/.phc files> [--dlt]\n", argv[0]);
        return 2;
    }
    const bool with_dlt = argc > 2 && !std::strcmp(argv[2], "--dlt");
    const auto t0 = std::chrono::steady_clock::now();
    try {
        std::unique_ptr<AiconProject> pr = read_aicon_flat(argv[1]);
        Camera &cam = *pr->camera;
        cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION)->get(3)->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCx()->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCy()->setColumn(COLUMN_FIXED);
        for (auto &p : pr->points)
            if (p->getName().size() > 3) p->setDatum(false);

        if (with_dlt) {                                                    // orientations from the DLT, one device call
            std::vector<std::unique_ptr<DLTCoefficients>> dlt;
            std::vector<DLTCoefficients *> all;
            for (auto &im : cam.images()) {
                dlt.emplace_back(new DLTCoefficients(im.get()));
                all.push_back(dlt.back().get());
            }
            DirectLinearTransformation::adjustAll(all, pr->byName);
            int failed = 0;
            for (DLTCoefficients *co : all) {
                if (co->status != JAICOV_DLT_CONVERGED && co->status != JAICOV_DLT_NOT_CONVERGED) { failed++; continue; }
                DirectLinearTransformation::applyExteriorOrientation(*co, co->getReference()->getExteriorOrientation());
            }
            std::printf("orientations                  DLT (%zu images, %d keep their .eor orientation)\n", all.size(), failed);
        } else {
            std::printf("orientations                  .eor\n");
        }

        // every object point from its image rays, one device call
        std::map<ObjectCoordinate *, std::array<double, 3>> obc;
        for (auto &p : pr->points) obc[p.get()] = {p->getX().getValue(), p->getY().getValue(), p->getZ().getValue()};
        const auto ti = std::chrono::steady_clock::now();
        const std::vector<ForwardIntersection::Result> res = ForwardIntersection::intersectAll({&cam});
        const double isect_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - ti).count();
        int count[5] = {0, 0, 0, 0, 0}, max_iter = 0;
        double maxd = 0.0, min_angle = M_PI;
        for (const ForwardIntersection::Result &r : res) {
            count[r.status]++;
            if (r.status != JAICOV_ISECT_OK && r.status != JAICOV_ISECT_NOT_CONVERGED) continue;
            const std::array<double, 3> &o = obc[r.point];
            maxd = std::max(maxd, std::sqrt((r.values[0] - o[0]) * (r.values[0] - o[0]) + (r.values[1] - o[1]) * (r.values[1] - o[1]) +
                                            (r.values[2] - o[2]) * (r.values[2] - o[2])));
            min_angle = std::min(min_angle, r.values[10]);
            max_iter = std::max(max_iter, r.iterations);
        }
        std::printf("intersected points            %zu (%.3f sec)\n", res.size(), isect_secs);
        std::printf("status ok / not converged     %d / %d\n", count[0], count[1]);
        std::printf("too few rays / singular / nan %d / %d / %d (these keep their .obc value)\n", count[2], count[3], count[4]);
        std::printf("most Gauss-Newton steps       %d\n", max_iter);
        std::printf("smallest largest ray angle    %.6f rad\n", min_angle);
        std::printf("max |intersected - obc|       %.6f mm\n", maxd);

        BundleAdjustment ba;
        ba.add(&cam);
        for (auto &s : pr->scaleBars) ba.add(s.get());
        ba.setInvertNormalEquation(MatrixInversion::REDUCED);
        ba.addPropertyChangeListener([](const std::string &name, double a, double b) {
            if (name == "CONVERGENCE") std::printf("  max|dx| = %.3e (threshold %.3e)\n", b, a);
        });
        const EstimationStateType state = ba.estimateModel();
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("state                      %d%s\n", (int)state, state == EstimationStateType::ERROR_FREE_ESTIMATION ? " (ERROR_FREE_ESTIMATION)" : "");
        if (!ba.lastError().empty()) std::printf("engine                     %s\n", ba.lastError().c_str());
        std::printf("iterations                 %d\n", ba.getIterations());
        std::printf("omega                      %.10e\n", ba.getOmega());
        std::printf("sigma0 a-posteriori        %.9f\n", std::sqrt(ba.getVarianceFactorAposteriori()));
        std::printf("Estimation time: %.3f sec\n", secs);
        return state == EstimationStateType::ERROR_FREE_ESTIMATION ? 0 : 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
