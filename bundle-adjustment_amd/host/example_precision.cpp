// The precision side of the bundled block's adjustment (include/jaicov_precision.h): reads the AICON flat files
// <base>.obc/.scale/.ior/.eor/.phc as example_flatfiles does, adjusts with MatrixInversion::FULL and prints, from the cofactor matrix
// on the device: the three object points with the largest Helmert point error with their confidence ellipsoids, the scale bars'
// lengths with their standard deviations, and the share of the trace that the first principal component of the point block takes.
// No Python, no oracle: C++ host mirror + libjaicov_neq.so only.
//   usage: example_precision <base path>
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <set>

#include "aicon_reader.hpp"

using namespace jaicov::host;

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
        std::printf("state                      %d%s\n", (int)state, state == EstimationStateType::ERROR_FREE_ESTIMATION ? " (ERROR_FREE_ESTIMATION)" : "");
        if (state != EstimationStateType::ERROR_FREE_ESTIMATION) {
            std::fprintf(stderr, "error: %s\n", ba.lastError().c_str());
            return 1;
        }
        const double s2 = ba.getVarianceFactorAposteriori();
        std::printf("sigma0 a-posteriori        %.9f\n", std::sqrt(s2));

        // 1. every object point; the three largest Helmert point errors
        const auto &ocs = ba.getObjectCoordinates();
        const BundleAdjustment::PrecisionTable pt = ba.pointPrecision(s2);
        std::vector<size_t> order(ocs.size());
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return pt.table[a * pt.columns + 3] > pt.table[b * pt.columns + 3]; });
        std::printf("object points              %zu\n", ocs.size());
        for (size_t r = 0; r < std::min<size_t>(3, order.size()); r++) {
            const double *o = &pt.table[order[r] * pt.columns];
            std::printf("point %-8s Helmert %.6f mm, sigma %.6f %.6f %.6f, status %d\n", ocs[order[r]]->getName().c_str(), o[3], o[0], o[1], o[2],
                        pt.status[order[r]]);
            for (int a = 0; a < 3; a++)
                std::printf("    semi-axis %.6f mm along (%+.6f %+.6f %+.6f)\n", o[4 + a], o[7 + 3 * a], o[8 + 3 * a], o[9 + 3 * a]);
            std::printf("    horizontal ellipse %.6f x %.6f mm, direction %.6f rad\n", o[16], o[17], o[18]);
        }

        // 2. the scale bars: adjusted length and its standard deviation from the 6 x 6 block of the two end points
        std::vector<int32_t> pairs;
        for (auto &s : pr->scaleBars) {
            pairs.push_back(s->getObjectCoordinateA()->index);
            pairs.push_back(s->getObjectCoordinateB()->index);
        }
        const BundleAdjustment::PrecisionTable len = ba.lengthPrecision(s2, pairs);
        for (size_t i = 0; i < pr->scaleBars.size(); i++)
            std::printf("scale bar %s - %s length %.6f mm, sigma %.6f mm (observed %.6f), status %d\n",
                        pr->scaleBars[i]->getObjectCoordinateA()->getName().c_str(), pr->scaleBars[i]->getObjectCoordinateB()->getName().c_str(),
                        len.table[i * len.columns], len.table[i * len.columns + 1], pr->scaleBars[i]->getLength().getValue(), len.status[i]);

        // 3. the weak form of the network: the first principal components of the block of the image-observed points
        std::set<int> cols;
        for (auto &im : cam.images())
            for (auto &ic : im->coordinates()) {
                ObjectCoordinate *p = ic->getObjectCoordinate();
                for (UnknownParameter *q : {&p->getX(), &p->getY(), &p->getZ()})
                    if (q->getColumn() >= 0) cols.insert(q->getColumn());
            }
        if (cols.empty() || *cols.rbegin() - *cols.begin() + 1 != (int)cols.size()) throw std::runtime_error("the point columns are not one range");
        const BundleAdjustment::PrincipalComponents pc = ba.principalComponents(*cols.begin(), (int)cols.size(), 3);
        std::printf("point block                columns %d .. %d, trace %.9e\n", *cols.begin(), *cols.rbegin(), pc.trace);
        std::printf("principal components       %s after %d products\n", pc.converged ? "converged" : "NOT converged", pc.iterations);
        for (size_t a = 0; a < pc.values.size(); a++)
            std::printf("component %zu share of the trace %.6f (eigenvalue %.9e, residual %.3e)\n", a + 1, pc.values[a] / pc.trace, pc.values[a],
                        pc.residuals[a]);
        return pc.converged ? 0 : 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
