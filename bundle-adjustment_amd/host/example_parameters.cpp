// The determinability of the additional parameters of the bundled block (include/jaicov_parameters.h): reads the AICON report as
// example_report does, adjusts with MatrixInversion::FULL and prints, from the cofactor matrix on the device, the report's two kinds
// of table in its layout -- the `Korrelation` matrix of the interior orientation and one `Korrelationen` table (exterior against
// interior orientation) per image, from ONE call of correlationBlock -- then value, sigma, t and worst partner of every interior and
// distortion parameter.  The report lists Ck, the adjustment estimates c = -Ck: the signs of Ck's correlations are flipped to the report's.
// No Python, no oracle: C++ host mirror + libjaicov_neq.so only.
//   usage: example_parameters <report.htm> [number of images to print, default 3]
#include <cstdio>
#include <cstdlib>
#include <map>

#include "aicon_reader.hpp"

using namespace jaicov::host;

static bool isFree(UnknownParameter *q) { return q && q->getColumn() >= 0 && q->getColumn() != COLUMN_FIXED; }

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <report.htm> [images to print]\n", argv[0]);
        return 2;
    }
    const int shown = argc > 2 ? std::atoi(argv[2]) : 3;
    try {
        std::unique_ptr<AiconProject> pr = read_aicon_report(argv[1]);
        if (pr->cameras.empty()) throw std::runtime_error("no interior orientation in the report");
        Camera &cam = *pr->cameras[0];
        for (auto &im : cam.images())
            for (auto &ic : im->coordinates())
                if (ic->getObjectCoordinate()->getName().size() > 3) ic->getObjectCoordinate()->setDatum(false);
        BundleAdjustment ba;
        import_report(ba, *pr);
        ba.setInvertNormalEquation(MatrixInversion::FULL);
        const EstimationStateType state = ba.estimateModel();
        if (state != EstimationStateType::ERROR_FREE_ESTIMATION) {
            std::fprintf(stderr, "error: %s\n", ba.lastError().c_str());
            return 1;
        }
        const double s2 = ba.getVarianceFactorAposteriori();
        std::printf("sigma0 a-posteriori        %.9f\n", std::sqrt(s2));

        // the free interior and distortion parameters under the report's names, in its order
        auto &io = cam.getInteriorOrientation();
        DistortionModel *rad = cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION);
        DistortionModel *tan = cam.getDistortionModel(DistortionModel::Type::TANGENTIAL_DISTORTION);
        DistortionModel *aff = cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR);
        std::vector<std::pair<const char *, UnknownParameter *>> all = {
            {"Ck", &io.getPrincipleDistance()}, {"Xh", &io.getPrinciplePointX()}, {"Yh", &io.getPrinciplePointY()},
            {"A1", rad ? rad->get(1) : nullptr}, {"A2", rad ? rad->get(2) : nullptr}, {"A3", rad ? rad->get(3) : nullptr},
            {"B1", tan ? tan->getBx() : nullptr}, {"B2", tan ? tan->getBy() : nullptr},
            {"C1", aff ? aff->getCx() : nullptr}, {"C2", aff ? aff->getCy() : nullptr}};
        std::vector<const char *> names;
        std::vector<int32_t> cols;
        std::vector<double> flip;
        for (auto &[name, q] : all)
            if (isFree(q)) {
                names.push_back(name);
                cols.push_back(q->getColumn());
                flip.push_back(q == &io.getPrincipleDistance() ? -1.0 : 1.0);
            }
        const int n = (int)cols.size();

        // 1. the report's `Korrelation` matrix
        const std::vector<double> R = ba.correlationBlock(cols, cols);
        std::printf("\nKorrelation:\n\n");
        for (int a = 0; a < n; a++) {
            std::printf("%-4s", names[a]);
            for (int b = 0; b <= a; b++) std::printf("  %6.3f", flip[a] * flip[b] * R[(size_t)a * n + b]);
            std::printf("\n");
        }
        std::printf("    ");
        for (int a = 0; a < n; a++) std::printf("  %6s", names[a]);
        std::printf("\n");

        // 2. the `Korrelationen` table of every image: all of them in one call
        std::vector<int32_t> rows;
        std::vector<long> ids;
        for (auto &im : cam.images()) {
            bool free6 = true;
            for (int k = 0; k < 6; k++) free6 = free6 && isFree(im->getExteriorOrientation().at(k));
            if (!free6) continue;
            ids.push_back(im->getId());
            for (int k = 0; k < 6; k++) rows.push_back(im->getExteriorOrientation().at(k)->getColumn());
        }
        const std::vector<double> K = ba.correlationBlock(rows, cols);
        static const char *eo_name[6] = {"x", "y", "z", "rx", "ry", "rz"};
        std::printf("\nimages                     %zu (%zu x %d coefficients from one call)\n", ids.size(), rows.size(), n);
        for (size_t i = 0; i < ids.size() && (int)i < shown; i++) {
            std::printf("\nimage %ld\n         Korrelationen:\n", ids[i]);
            for (int k = 0; k < 6; k++) {
                std::printf("          %2s ", eo_name[k]);
                for (int b = 0; b < n; b++) std::printf("  %6.3f", flip[b] * K[((size_t)6 * i + k) * n + b]);
                std::printf("\n");
            }
            std::printf("             ");
            for (int b = 0; b < n; b++) std::printf("  %6s", names[b]);
            std::printf("\n");
        }

        // 3. value, sigma, t and worst partner of every interior and distortion parameter
        std::map<UnknownParameter *, int32_t> slot_of;
        for (size_t s = 0; s < ba.flat.slot_param.size(); s++) slot_of[ba.flat.slot_param[s]] = (int32_t)s;
        std::vector<int32_t> begin = {0}, slots;
        for (auto &[name, q] : all)
            if (q) { slots.push_back(slot_of.at(q)); begin.push_back((int32_t)slots.size()); }
        const BundleAdjustment::ParameterTests t = ba.testParameters(s2, begin, slots);
        const uint32_t inner = 1u << (4 * JAICOV_PAR_CLASS_INTERIOR + JAICOV_PAR_CLASS_INTERIOR) | 1u << (4 * JAICOV_PAR_CLASS_INTERIOR + JAICOV_PAR_CLASS_DISTORTION) |
                               1u << (4 * JAICOV_PAR_CLASS_DISTORTION + JAICOV_PAR_CLASS_INTERIOR) | 1u << (4 * JAICOV_PAR_CLASS_DISTORTION + JAICOV_PAR_CLASS_DISTORTION);
        const BundleAdjustment::ParameterCorrelations worst = ba.parameterCorrelations(inner, 0);
        const uint32_t to_eo = 1u << (4 * JAICOV_PAR_CLASS_INTERIOR + JAICOV_PAR_CLASS_EXTERIOR) | 1u << (4 * JAICOV_PAR_CLASS_DISTORTION + JAICOV_PAR_CLASS_EXTERIOR);
        const BundleAdjustment::ParameterCorrelations worst_eo = ba.parameterCorrelations(to_eo, 0);
        std::printf("\n");
        int g = 0;
        for (auto &[name, q] : all) {
            if (!q) continue;
            const double *o = &t.table[(size_t)JAICOV_PAR_TEST_COLUMNS * g];
            if (t.status[g] & JAICOV_PAR_EMPTY) {
                std::printf("parameter %-3s %+.6e  fest\n", name, q->getValue());
            } else {
                const int c = q->getColumn();
                const char *pn = "-";
                for (int b = 0; b < n; b++)
                    if (cols[b] == worst.partner[c]) pn = names[b];
                const double sign = (q == &io.getPrincipleDistance()) != (worst.partner[c] == io.getPrincipleDistance().getColumn()) ? -1.0 : 1.0;
                std::printf("parameter %-3s %+.6e  sigma %.6e  t %+.1f  worst partner %s rho %+.3f, among the exterior orientations column %d rho %+.3f, status %d\n",
                            name, q->getValue(), std::sqrt(s2 * ba.cofactor(c, c)), o[3], pn, sign * worst.rho[c], worst_eo.partner[c],
                            worst_eo.rho[c], t.status[g]);
            }
            ++g;
        }
        const BundleAdjustment::CorrelatedPairs strong = ba.correlatedPairs(0.9, inner | to_eo, 0, 1 << 12);
        std::printf("pairs with |rho| >= 0.9 among interior, distortion and against the exterior orientations: %lld\n", (long long)strong.count);
        return 0;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
