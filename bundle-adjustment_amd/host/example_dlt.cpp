// The bundled block adjusted from DLT start values: reads the AICON flat files <base>.obc/.scale/.ior/.eor/.phc as example_flatfiles
// does, replaces every image's exterior orientation from the .eor file by the DLT's (DirectLinearTransformation::adjustAll, one device
// call for all images, the .obc coordinates as control), prints the DLT-versus-.eor differences per image, then runs estimateModel()
// and prints the listing of example_flatfiles.  The camera's c < 0 (AICON), so the start values take quirk Q1 (kappa + pi).
//   usage: example_dlt <base path> [FULL|REDUCED|PRE_ELIMINATION|NONE]
#include <chrono>
#include <cstdio>
#include <cstring>

#include "aicon_reader.hpp"

using namespace jaicov::host;

static double wrap(double a) {   // into (-pi, pi]
    while (a > M_PI) a -= 2.0 * M_PI;
    while (a <= -M_PI) a += 2.0 * M_PI;
    return a;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <base path of the .obc/.scale/.ior/.eor/.phc files> [FULL|REDUCED|PRE_ELIMINATION|NONE]\n", argv[0]);
        return 2;
    }
    const auto t0 = std::chrono::steady_clock::now();
    MatrixInversion inv = MatrixInversion::FULL;
    if (argc > 2) {
        if (!std::strcmp(argv[2], "REDUCED")) inv = MatrixInversion::REDUCED;
        else if (!std::strcmp(argv[2], "PRE_ELIMINATION")) inv = MatrixInversion::PRE_ELIMINATION;
        else if (!std::strcmp(argv[2], "NONE")) inv = MatrixInversion::NONE;
    }
    try {
        std::unique_ptr<AiconProject> pr = read_aicon_flat(argv[1]);
        Camera &cam = *pr->camera;
        cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION)->get(3)->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCx()->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCy()->setColumn(COLUMN_FIXED);
        for (auto &p : pr->points)
            if (p->getName().size() > 3) p->setDatum(false);

        // DLT start values for every image in one device call
        std::vector<std::unique_ptr<DLTCoefficients>> dlt;
        std::vector<DLTCoefficients *> all;
        for (auto &im : cam.images()) {
            dlt.emplace_back(new DLTCoefficients(im.get()));
            all.push_back(dlt.back().get());
        }
        const auto td = std::chrono::steady_clock::now();
        DirectLinearTransformation::adjustAll(all, pr->byName);
        const double dlt_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - td).count();
        std::printf("DLT start values (%zu images, %.3f sec), differences to the .eor orientation:\n", all.size(), dlt_secs);
        std::printf("  image status solves      dX0 [mm]     dY0 [mm]     dZ0 [mm]   domega [rad]     dphi [rad]   dkappa [rad]\n");
        double maxd = 0.0, maxa = 0.0;
        int failed = 0;
        for (DLTCoefficients *co : all) {
            Image *im = co->getReference();
            ExteriorOrientation &eo = im->getExteriorOrientation();
            double before[6], after[6];
            for (int i = 0; i < 6; i++) before[i] = eo.at(i)->getValue();
            if (co->status != JAICOV_DLT_CONVERGED && co->status != JAICOV_DLT_NOT_CONVERGED) {
                std::printf("  %5ld %6d %6d  (no DLT result: the .eor orientation is kept)\n", im->getId(), co->status, co->solves);
                failed++;
                continue;
            }
            DirectLinearTransformation::applyExteriorOrientation(*co, eo);
            for (int i = 0; i < 6; i++) after[i] = eo.at(i)->getValue();
            double d[6];
            for (int i = 0; i < 3; i++) { d[i] = after[i] - before[i]; maxd = std::max(maxd, std::fabs(d[i])); }
            for (int i = 3; i < 6; i++) { d[i] = wrap(after[i] - before[i]); maxa = std::max(maxa, std::fabs(d[i])); }
            std::printf("  %5ld %6d %6d %12.4f %12.4f %12.4f %14.3e %14.3e %14.3e\n", im->getId(), co->status, co->solves, d[0], d[1], d[2],
                        d[3], d[4], d[5]);
        }
        std::printf("max |DLT - eor| X0            %.6f mm\n", maxd);
        std::printf("max |DLT - eor| angle         %.6e rad\n", maxa);
        std::printf("images without DLT result     %d\n", failed);

        BundleAdjustment ba;
        ba.add(&cam);
        for (auto &s : pr->scaleBars) ba.add(s.get());
        ba.setInvertNormalEquation(inv);
        ba.addPropertyChangeListener([](const std::string &name, double a, double b) {
            if (name == "CONVERGENCE") std::printf("  max|dx| = %.3e (threshold %.3e)\n", b, a);
        });
        const EstimationStateType state = ba.estimateModel();
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("state                      %d%s\n", (int)state, state == EstimationStateType::ERROR_FREE_ESTIMATION ? " (ERROR_FREE_ESTIMATION)" : "");
        if (!ba.lastError().empty()) std::printf("engine                     %s\n", ba.lastError().c_str());
        std::printf("observations               %d\n", ba.getNumberOfObservations());
        std::printf("unknown parameters         %d\n", ba.getNumberOfUnknownParameters());
        std::printf("datum conditions           %d\n", ba.getNumberOfDatumConditions());
        std::printf("degree of freedom          %d\n", ba.getDegreeOfFreedom());
        std::printf("iterations                 %d\n", ba.getIterations());
        std::printf("omega                      %.10e\n", ba.getOmega());
        std::printf("sigma0 a-posteriori        %.9f\n", std::sqrt(ba.getVarianceFactorAposteriori()));
        auto &io = cam.getInteriorOrientation();
        std::printf("c, x0, y0                  %.6f %.6f %.6f\n", io.getPrincipleDistance().getValue(), io.getPrinciplePointX().getValue(),
                    io.getPrinciplePointY().getValue());
        if (inv != MatrixInversion::NONE && !ba.getObjectCoordinates().empty()) {
            ObjectCoordinate *p = ba.getObjectCoordinates().front();
            const double s2 = ba.getVarianceFactorAposteriori();
            std::printf("point %-8s            %.5f %.5f %.5f  +/- %.5f %.5f %.5f\n", p->getName().c_str(), p->getX().getValue(),
                        p->getY().getValue(), p->getZ().getValue(), std::sqrt(s2 * ba.cofactor(p->getX().getColumn(), p->getX().getColumn())),
                        std::sqrt(s2 * ba.cofactor(p->getY().getColumn(), p->getY().getColumn())),
                        std::sqrt(s2 * ba.cofactor(p->getZ().getColumn(), p->getZ().getColumn())));
        }
        std::printf("Estimation time: %.3f sec\n", secs);
        return state == EstimationStateType::ERROR_FREE_ESTIMATION ? 0 : 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
