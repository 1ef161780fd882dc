// The stochastic model of the bundled block put to the test (include/jaicov_vce.h): reads the AICON flat files
// <base>.obc/.scale/.ior/.eor/.phc as example_flatfiles does, adjusts the block with MatrixInversion::FULL and prints the variance
// components by kind (image points, scale bars, directly observed rows) and the ten images whose image points ask for the largest
// factor on their dispersions (groups by image).
// No Python, no oracle: C++ host mirror + libjaicov_neq.so only.
//   usage: example_variance_components <base path>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <stdexcept>

#include "aicon_reader.hpp"

using namespace jaicov::host;

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <base path of the .obc/.scale/.ior/.eor/.phc files>\n", argv[0]);
        return 2;
    }
    try {
        const std::string base = argv[1];
        std::unique_ptr<AiconProject> owner(new AiconProject());
        AiconProject &pr = *owner;
        read_obc(pr, base + ".obc");
        read_ior(pr, base + ".ior");
        read_scale(pr, base + ".scale");
        read_eor(pr, base + ".eor");
        for_each_line(base + ".phc", [&](const std::string &line) {                     // PHCFileReader.java:74-117
            auto col = split_ws(line);
            if (col.size() < 11 || !(std::stoi(col[9]) > 0)) return;
            Image *im = pr.camera->add(std::stol(col[0]));
            auto it = pr.byName.find(col[1]);
            if (it == pr.byName.end()) return;
            im->add(it->second, std::stod(col[2]), std::stod(col[3]), std::stod(col[4]), std::stod(col[5]));
        });
        Camera &cam = *pr.camera;
        cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION)->get(3)->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCx()->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCy()->setColumn(COLUMN_FIXED);
        for (auto &p : pr.points)
            if (p->getName().size() > 3) p->setDatum(false);
        BundleAdjustment ba;
        ba.add(&cam);
        for (auto &s : pr.scaleBars) ba.add(s.get());
        ba.setInvertNormalEquation(MatrixInversion::FULL);
        const EstimationStateType state = ba.estimateModel();
        if (state != EstimationStateType::ERROR_FREE_ESTIMATION) {
            std::fprintf(stderr, "error: %s\n", ba.lastError().c_str());
            return 1;
        }
        std::printf("sigma2 a-priori %.6g, a-posteriori %.6g, degrees of freedom %d\n", ba.getVarianceFactorApriori(), ba.getVarianceFactorAposteriori(),
                    ba.getDegreeOfFreedom());
        auto print = [](const char *name, const BundleAdjustment::VarianceComponents &c, size_t g) {
            const size_t G = c.status.size();
            std::printf("%-16s %8.0f %14.6g %12.4f %12.6g %10.4f %8.4f  %d\n", name, c.table[g], c.table[G + g], c.table[2 * G + g], c.table[3 * G + g],
                        c.table[4 * G + g], c.table[5 * G + g], c.status[g]);
        };
        const char *head = "group                rows          Omega            r           s2          k    sd(k)  status\n";
        const BundleAdjustment::VarianceComponents kind = ba.varianceComponents(ba.varianceGroupsByKind());
        std::printf("%s", head);
        const char *names[3] = {"image points", "scale bars", "direct rows"};
        for (size_t g = 0; g < 3; g++) print(names[g], kind, g);
        std::printf("all rows: Omega %.6g, sum r %.4f (damping of the inverted build %.3g), %0.f rows in groups, %0.f in none\n", kind.omega, kind.sumR,
                    kind.damping, kind.rowsGrouped, kind.rowsUngrouped);
        const BundleAdjustment::VarianceComponents img = ba.varianceComponents(ba.varianceGroupsByImage());
        const size_t I = img.status.size();
        std::vector<size_t> order(I);
        std::iota(order.begin(), order.end(), 0);
        auto key = [&](size_t g) { return img.status[g] ? -1.0 : img.k((int)g); };
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return key(a) > key(b) || (key(a) == key(b) && a < b); });
        std::printf("the ten images with the largest factor\n%s", head);
        size_t shown = 0;
        for (size_t o = 0; o < I && shown < 10; o++, shown++) {
            char name[32];
            std::snprintf(name, sizeof name, "image %zu", order[o]);
            print(name, img, order[o]);
        }
        // by kind every row is in a group: the groups add up to the totals, and these to the degrees of freedom of an undamped build
        const double sumR = kind.table[2 * 3] + kind.table[2 * 3 + 1] + kind.table[2 * 3 + 2];
        const bool ok = kind.rowsUngrouped == 0 && std::fabs(sumR - kind.sumR) <= 1e-9 * std::fabs(kind.sumR) &&
                        (kind.damping != 0.0 || std::fabs(kind.sumR - ba.getDegreeOfFreedom()) <= 1e-6 * ba.getDegreeOfFreedom());
        return ok ? 0 : 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
