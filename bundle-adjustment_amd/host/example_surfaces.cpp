// Cylinders and cones through adjusted points of the bundled block (include/jaicov_surfaces.h): reads the AICON flat files
// <base>.obc/.scale/.ior/.eor/.phc as example_flatfiles does, adjusts with MatrixInversion::FULL and fits, on the device and with the
// members' whole block of the cofactor matrix, a cylinder to the first 16 object points of the file and a cone to the next 12, each
// from start values of its own (the search over candidate axes).  The cylinder is then fitted once more from the first result as a
// given start.  The points do not lie on such surfaces: the listing shows what the call returns and agrees with the Python route.
// No Python, no oracle: C++ host mirror + libjaicov_neq.so only.
//   usage: example_surfaces <base path>
#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "aicon_reader.hpp"

using namespace jaicov::host;

static void list(const char *name, const BundleAdjustment::FormFits &f, int g, const std::vector<int32_t> &begin, const std::vector<int32_t> &point) {
    const double *o = &f.table[(size_t)JAICOV_FORM_COLUMNS * g];
    std::printf("form %s status %d iterations %d members", name, f.status[g], (int)o[19]);
    for (int i = begin[g]; i < begin[g + 1]; i++) std::printf(" %d", point[i]);
    std::printf("\n  parameters");
    for (int a = 0; a < 7; a++) std::printf(" %.17g", o[a]);
    std::printf("\n  sigma");
    for (int a = 0; a < 7; a++) std::printf(" %.17g", o[7 + a]);
    std::printf("\n  Omega %.17g f %.17g T %.17g largest distance %.17g rms %.17g\n", o[14], o[15], o[16], o[17], o[18]);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <base path of the .obc/.scale/.ior/.eor/.phc files>\n", argv[0]);
        return 2;
    }
    try {
        std::unique_ptr<AiconProject> pr = read_aicon_flat(argv[1]);
        Camera &cam = *pr->camera;
        cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION)->get(3)->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCx()->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCy()->setColumn(COLUMN_FIXED);
        for (auto &p : pr->points)
            if (p->getName().size() > 3) p->setDatum(false);
        BundleAdjustment ba;
        ba.add(&cam);
        for (auto &s : pr->scaleBars) ba.add(s.get());
        ba.setInvertNormalEquation(MatrixInversion::FULL);
        const EstimationStateType state = ba.estimateModel();
        if (state != EstimationStateType::ERROR_FREE_ESTIMATION) {
            std::fprintf(stderr, "error: %s\n", ba.lastError().c_str());
            return 1;
        }
        const double s2 = ba.getVarianceFactorAposteriori();
        std::printf("sigma2 a-posteriori %.17g\n", s2);
        if (pr->points.size() < 28) throw std::runtime_error("fewer than 28 object points in the file");
        const std::vector<int32_t> type = {JAICOV_SURF_CYLINDER, JAICOV_SURF_CONE}, begin = {0, 16, 28};
        std::vector<int32_t> point;
        for (size_t i = 0; i < 28; i++) point.push_back(pr->points[i]->index);
        const BundleAdjustment::FormFits f = ba.fitSurfaces(s2, type, begin, point, {}, 50);
        list("cylinder", f, 0, begin, point);
        list("cone", f, 1, begin, point);
        // the cylinder once more, from the result as a given start; the cone finds its own again (a row that begins with NaN)
        std::vector<double> start(14, NAN);
        bool usable = true;
        for (int a = 0; a < 7; a++) usable = usable && std::isfinite(f.table[a]);
        if (usable)
            for (int a = 0; a < 7; a++) start[a] = f.table[a];
        const BundleAdjustment::FormFits again = ba.fitSurfaces(s2, type, begin, point, start, 50);
        list("cylinder_from_start", again, 0, begin, point);
        return 0;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
