// The bundled block adjusted from start values that come from its image measurements and the .ior camera alone: reads the AICON flat
// files <base>.obc/.scale/.ior/.eor/.phc as example_flatfiles does and ignores the .obc coordinates and the .eor orientations.
//   1. the pair of images with the most common points is oriented relatively (RelativeOrientation::orientAll, base length 1);
//   2. every point that at least two oriented images see is intersected from those images (jaicov_isect_points);
//   3. every image not yet oriented that sees at least 6 intersected points is resected from them (jaicov_resect_images), and
//      where none does, every one that sees at least 4;
//   2 and 3 alternate until no image is added, then every point is intersected from all oriented images;
//   4. the model is scaled so that the first scale bar has its length, and estimateModel() runs with MatrixInversion::REDUCED.
// Steps 1 to 3 are model_growth.hpp's, which example_absolute shares.
//   usage: example_relative <base path>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "model_growth.hpp"

using namespace jaicov::host;

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <base path of the .obc/.scale/.ior/.eor/.phc files>\n", argv[0]);
        return 2;
    }
    const auto t0 = std::chrono::steady_clock::now();
    try {
        std::unique_ptr<AiconProject> pr = read_aicon_flat(argv[1]);
        Camera &cam = *pr->camera;
        cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION)->get(3)->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCx()->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCy()->setColumn(COLUMN_FIXED);
        for (auto &p : pr->points)
            if (p->getName().size() > 3) p->setDatum(false);
        growth::grow_model(*pr, cam);                                         // steps 1 to 3, reported line by line

        // 4. the scale of the first scale bar
        if (pr->scaleBars.empty()) throw std::runtime_error("no scale bar");
        ScaleBar &bar = *pr->scaleBars[0];
        ObjectCoordinate *A = bar.getObjectCoordinateA(), *B = bar.getObjectCoordinateB();
        const double dx = A->getX().getValue() - B->getX().getValue(), dy = A->getY().getValue() - B->getY().getValue(),
                     dz = A->getZ().getValue() - B->getZ().getValue();
        const double f = bar.getLength().getValue() / std::sqrt(dx * dx + dy * dy + dz * dz);
        for (auto &p : pr->points) {
            p->getX().setValue(f * p->getX().getValue()); p->getY().setValue(f * p->getY().getValue()); p->getZ().setValue(f * p->getZ().getValue());
        }
        for (auto &im : cam.images())
            for (int k = 0; k < 3; k++) im->getExteriorOrientation().at(k)->setValue(f * im->getExteriorOrientation().at(k)->getValue());
        std::printf("scale (base length)           %.6f\n", f);
        std::printf("start values                  %.3f sec\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());

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
