// jaicov.cpp -- host-side driver logic of the JAICOV mirror (see jaicov.hpp).  Control and integer work only; all
// per-iteration arithmetic goes through the C ABI (include/jaicov_neq.h) to the MI355X.
#include "jaicov.hpp"

#include <cstring>

namespace jaicov::host {

static const double SQRT_EPS = std::sqrt(1.1102230246251565e-16);   // sqrt(Constant.EPS), BundleAdjustment.java:77

// ---------------------------------------------------------------------------------------------------------------
// BundleAdjustment.prepareUnknownParameters (BundleAdjustment.java:667-782), loop for loop
// ---------------------------------------------------------------------------------------------------------------
void BundleAdjustment::prepareUnknownParameters() {
    if (prepared_) throw std::logic_error("estimateModel() is single-shot (BundleAdjustment.java:80-83,776-781)");
    prepared_ = true;
    for (Camera *camera : cameras_)
        for (auto &image : camera->images())
            for (auto &ic : image->coordinates()) {
                ic->getX().setRow(numberOfObservations_++);
                ic->getY().setRow(numberOfObservations_++);
                ObjectCoordinate *oc = ic->getObjectCoordinate();
                addObjectCoordinate(oc);
                addUnknownParameter(&oc->getX());
                addUnknownParameter(&oc->getY());
                addUnknownParameter(&oc->getZ());
                noteVariance(ic->getX().getVariance());
                noteVariance(ic->getY().getVariance());
            }
    for (Camera *camera : cameras_) {
        for (int i = 0; i < 3; i++) addUnknownParameter(camera->getInteriorOrientation().at(i));
        for (auto &model : camera->getDistortionModels())
            for (auto &p : model->parameters()) addUnknownParameter(p.get());
    }
    for (Camera *camera : cameras_)
        for (auto &image : camera->images())
            for (int i = 0; i < 6; i++) addUnknownParameter(image->getExteriorOrientation().at(i));
    for (ScaleBar *sb : scaleBars_) {
        sb->getLength().setRow(numberOfObservations_++);
        ObjectCoordinate *a = sb->getObjectCoordinateA(), *b = sb->getObjectCoordinateB();
        addObjectCoordinate(a);
        addObjectCoordinate(b);
        addUnknownParameter(&a->getX()); addUnknownParameter(&a->getY()); addUnknownParameter(&a->getZ());
        addUnknownParameter(&b->getX()); addUnknownParameter(&b->getY()); addUnknownParameter(&b->getZ());
        noteVariance(sb->getLength().getVariance());
    }
    for (DirectlyObservedParameterGroup *g : groups_) {
        for (ObservationParameter *op : g->observations()) {
            UnknownParameter *up = op->getReferenceParameter();
            switch (up->getParameterType()) {
            case ParameterType::OBJECT_COORDINATE_X:
            case ParameterType::OBJECT_COORDINATE_Y:
            case ParameterType::OBJECT_COORDINATE_Z:
                addObjectCoordinate(static_cast<ObjectCoordinate *>(up->getReference()));
                break;
            default:
                break;
            }
            addUnknownParameter(up);
            op->setRow(numberOfObservations_++);
            noteVariance(op->getVariance());
        }
    }
    detectRankDefect();
    const int d = rankDefect_.getDefect();
    if (d > 0)
        for (UnknownParameter *p : unknownParameters_) p->setColumn(p->getColumn() + d);
}

// BundleAdjustment.detectRankDefect (BundleAdjustment.java:836-1042), literal
void BundleAdjustment::detectRankDefect() {
    using DT = RankDefect::DefectType;
    const bool hasScaleBars = !scaleBars_.empty();
    RankDefect &rd = rankDefect_;
    rd.reset();
    rd.setTranslationX(DT::FREE); rd.setTranslationY(DT::FREE); rd.setTranslationZ(DT::FREE);
    rd.setRotationX(DT::FREE); rd.setRotationY(DT::FREE); rd.setRotationZ(DT::FREE);
    rd.setScale(hasScaleBars ? DT::FIXED : DT::FREE);
    int kx = 0, ky = 0, kz = 0;
    if (rd.allFixed()) return;
    for (auto *g : groups_) {
        for (ObservationParameter *op : g->observations()) {
            switch (op->getParameterType()) {
            case ParameterType::CAMERA_OMEGA: rd.setRotationX(DT::FIXED); break;
            case ParameterType::CAMERA_PHI: rd.setRotationY(DT::FIXED); break;
            case ParameterType::CAMERA_KAPPA: rd.setRotationZ(DT::FIXED); break;
            default: break;
            }
            if (!rd.estimateRotationX() && !rd.estimateRotationY() && !rd.estimateRotationZ()) break;
        }
    }
    auto theory = [&]() {
        if (rd.estimateTranslationX() && kx > 0) rd.setTranslationX(DT::FIXED);
        if (rd.estimateTranslationY() && ky > 0) rd.setTranslationY(DT::FIXED);
        if (rd.estimateTranslationZ() && kz > 0) rd.setTranslationZ(DT::FIXED);
        if (!hasScaleBars && (kx >= 2 || ky >= 2 || kz >= 2)) rd.setScale(DT::FIXED);
        if (rd.estimateRotationX() && ky >= 2 && kz >= 2) rd.setRotationX(DT::FIXED);
        if (rd.estimateRotationY() && kx >= 2 && kz >= 2) rd.setRotationY(DT::FIXED);
        if (rd.estimateRotationZ() && kx >= 2 && ky >= 2) rd.setRotationZ(DT::FIXED);
        if (kx > 0 && ky > 0 && kz > 0 && ((hasScaleBars && kx + ky + kz >= 6) || (!hasScaleBars && kx + ky + kz >= 7))) {
            rd.setRotationX(DT::FIXED); rd.setRotationY(DT::FIXED); rd.setRotationZ(DT::FIXED);
        }
    };
    for (auto *g : groups_) {
        for (ObservationParameter *op : g->observations()) {
            switch (op->getParameterType()) {
            case ParameterType::CAMERA_COORDINATE_X: case ParameterType::OBJECT_COORDINATE_X: kx++; break;
            case ParameterType::CAMERA_COORDINATE_Y: case ParameterType::OBJECT_COORDINATE_Y: ky++; break;
            case ParameterType::CAMERA_COORDINATE_Z: case ParameterType::OBJECT_COORDINATE_Z: kz++; break;
            case ParameterType::CAMERA_OMEGA: rd.setRotationX(DT::FIXED); break;
            case ParameterType::CAMERA_PHI: rd.setRotationY(DT::FIXED); break;
            case ParameterType::CAMERA_KAPPA: rd.setRotationZ(DT::FIXED); break;
            default: break;
            }
            theory();
            if (rd.allFixed()) break;
        }
    }
    for (ObjectCoordinate *oc : objectCoordinates_) {
        kx += oc->getX().getColumn() == COLUMN_FIXED ? 1 : 0;
        ky += oc->getY().getColumn() == COLUMN_FIXED ? 1 : 0;
        kz += oc->getZ().getColumn() == COLUMN_FIXED ? 1 : 0;
        theory();
        if (rd.allFixed()) break;
    }
    if (rd.allFixed()) return;
    for (Camera *camera : cameras_) {
        for (auto &image : camera->images()) {
            ExteriorOrientation &eo = image->getExteriorOrientation();
            if (rd.estimateRotationX() && eo.get(ParameterType::CAMERA_OMEGA).getColumn() == COLUMN_FIXED) rd.setRotationX(DT::FIXED);
            if (rd.estimateRotationY() && eo.get(ParameterType::CAMERA_PHI).getColumn() == COLUMN_FIXED) rd.setRotationY(DT::FIXED);
            if (rd.estimateRotationZ() && eo.get(ParameterType::CAMERA_KAPPA).getColumn() == COLUMN_FIXED) rd.setRotationZ(DT::FIXED);
            kx += eo.get(ParameterType::CAMERA_COORDINATE_X).getColumn() == COLUMN_FIXED ? 1 : 0;
            ky += eo.get(ParameterType::CAMERA_COORDINATE_Y).getColumn() == COLUMN_FIXED ? 1 : 0;
            kz += eo.get(ParameterType::CAMERA_COORDINATE_Z).getColumn() == COLUMN_FIXED ? 1 : 0;
            theory();
            if (rd.allFixed()) break;
        }
        if (rd.allFixed()) break;
    }
}

// BundleAdjustment.centroidCoordinates (BundleAdjustment.java:115-201)
void BundleAdjustment::centroidCoordinates(bool invert) {
    auto axis = [](ParameterType t) {
        switch (t) {
        case ParameterType::CAMERA_COORDINATE_X: case ParameterType::OBJECT_COORDINATE_X: return 0;
        case ParameterType::CAMERA_COORDINATE_Y: case ParameterType::OBJECT_COORDINATE_Y: return 1;
        case ParameterType::CAMERA_COORDINATE_Z: case ParameterType::OBJECT_COORDINATE_Z: return 2;
        default: return -1;
        }
    };
    if (!invert) {
        double s[3] = {0, 0, 0};
        int cnt[3] = {0, 0, 0};
        for (UnknownParameter *p : unknownParameters_) {
            const int a = axis(p->getParameterType());
            if (a >= 0) { s[a] += p->getValue(); cnt[a]++; }
        }
        if (cnt[0] == cnt[1] && cnt[0] == cnt[2] && cnt[0] > 0) {
            for (int a = 0; a < 3; a++) centroid_[a] = s[a] / cnt[a];
        } else
            throw std::logic_error("Error, the numbers of coordinate components are un-equal or zero (BundleAdjustment.java:151)");
    }
    const double sign = invert ? 1.0 : -1.0;
    const double c[3] = {sign * centroid_[0], sign * centroid_[1], sign * centroid_[2]};
    for (UnknownParameter *p : unknownParameters_) {
        const int a = axis(p->getParameterType());
        if (a >= 0) p->setValue(p->getValue() + c[a]);
    }
    for (auto *g : groups_)
        for (ObservationParameter *op : g->observations()) {
            const int a = axis(op->getParameterType());
            if (a >= 0) op->setValue(op->getValue() + c[a]);
        }
}

// ---------------------------------------------------------------------------------------------------------------
// object graph -> flat arrays of jaicov_problem_desc
// ---------------------------------------------------------------------------------------------------------------
static int32_t flat_col(const UnknownParameter *p) {
    const int c = p->getColumn();
    return (c == COLUMN_FIXED || c < 0) ? JAICOV_COL_FIXED : c;
}

void BundleAdjustment::flatten() {
    Flat &f = flat;
    f = Flat();
    const int P = (int)objectCoordinates_.size();
    for (int i = 0; i < P; i++) objectCoordinates_[i]->index = i;
    int nimg = 0, ncam = 0;
    for (Camera *c : cameras_) {
        c->index = ncam++;
        for (auto &im : c->images()) im->index = nimg++;
    }
    // slots: points | io | dist | eo
    f.slot_param.clear();
    for (ObjectCoordinate *oc : objectCoordinates_) {
        UnknownParameter *q[3] = {&oc->getX(), &oc->getY(), &oc->getZ()};
        for (auto *p : q) { p->slot = (int)f.slot_param.size(); f.slot_param.push_back(p); f.point_col.push_back(flat_col(p)); }
        f.point_datum.push_back(oc->isDatum() ? 1 : 0);
    }
    for (Camera *c : cameras_)
        for (int i = 0; i < 3; i++) {
            UnknownParameter *p = c->getInteriorOrientation().at(i);
            p->slot = (int)f.slot_param.size(); f.slot_param.push_back(p); f.io_col.push_back(flat_col(p));
        }
    f.cam_dist_begin.push_back(0);
    for (Camera *c : cameras_) {
        double r0 = 0.0;
        for (auto &m : c->getDistortionModels()) {
            if (m->getType() >= DistortionModel::Type::RADIAL_DISTORTION) r0 = m->getR0();   // radial, distance, Zernike models carry r0
            for (auto &p : m->parameters()) {
                int kind;
                switch (p->getParameterType()) {
                case ParameterType::AFFINITY_AND_SHEAR_Cx: kind = JAICOV_DIST_AFFINITY_CX; break;
                case ParameterType::AFFINITY_AND_SHEAR_Cy: kind = JAICOV_DIST_AFFINITY_CY; break;
                case ParameterType::TANGENTIAL_DISTORTION_Bx: kind = JAICOV_DIST_TANGENTIAL_BX; break;
                case ParameterType::TANGENTIAL_DISTORTION_By: kind = JAICOV_DIST_TANGENTIAL_BY; break;
                case ParameterType::TANGENTIAL_POLYNOMIAL_B: kind = JAICOV_DIST_TANGENTIAL_BI; break;
                case ParameterType::RADIAL_POLYNOMIAL_A: kind = JAICOV_DIST_RADIAL_AI; break;
                case ParameterType::ZERNIKE_POLYNOMIAL_X: kind = JAICOV_DIST_ZERNIKE_X; break;
                case ParameterType::ZERNIKE_POLYNOMIAL_Y: kind = JAICOV_DIST_ZERNIKE_Y; break;
                case ParameterType::ZERNIKE_POLYNOMIAL_Z: kind = JAICOV_DIST_ZERNIKE_Z; break;
                default: kind = JAICOV_DIST_DISTANCE_DI; break;
                }
                p->slot = (int)f.slot_param.size(); f.slot_param.push_back(p.get());
                f.dist_kind.push_back(kind); f.dist_order.push_back(p->getOrder() > 0 ? p->getOrder() : 0); f.dist_col.push_back(flat_col(p.get()));
            }
        }
        f.cam_r0.push_back(r0);
        f.cam_dist_begin.push_back((int32_t)f.dist_kind.size());
    }
    for (Camera *c : cameras_)
        for (auto &im : c->images()) {
            f.image_camera.push_back(c->index);
            for (int i = 0; i < 6; i++) {
                UnknownParameter *p = im->getExteriorOrientation().at(i);
                p->slot = (int)f.slot_param.size(); f.slot_param.push_back(p); f.eo_col.push_back(flat_col(p));
            }
        }
    // image points, image-major; images with a joint dispersion become image blocks
    f.blk_ip_begin.clear();
    bool any_block = false, block_open = false;
    for (Camera *c : cameras_)
        for (auto &im : c->images()) {
            const bool blk = !im->dispersion().empty();
            if (blk) {
                if (any_block && !block_open) throw std::invalid_argument("images with a joint dispersion must be consecutive");
                if (!any_block) f.blk_ip_begin.push_back((int32_t)f.ip_image.size());
                any_block = block_open = true;
                f.blk_disp_offset.push_back((int64_t)f.blk_disp.size());
                f.blk_disp.insert(f.blk_disp.end(), im->dispersion().begin(), im->dispersion().end());
            } else if (block_open) block_open = false;
            for (auto &ic : im->coordinates()) {
                f.ip_image.push_back(im->index);
                f.ip_point.push_back(ic->getObjectCoordinate()->index);
                f.ip_x.push_back(ic->getX().getValue()); f.ip_y.push_back(ic->getY().getValue());
                f.ip_var_x.push_back(ic->getX().getVariance()); f.ip_var_y.push_back(ic->getY().getVariance());
                f.ip_rho.push_back(ic->getCorrelationCoefficientXY());
            }
            if (blk) f.blk_ip_begin.push_back((int32_t)f.ip_image.size());
        }
    if (!any_block) f.blk_ip_begin.push_back(0);
    for (ScaleBar *sb : scaleBars_) {
        f.sb_a.push_back(sb->getObjectCoordinateA()->index); f.sb_b.push_back(sb->getObjectCoordinateB()->index);
        f.sb_len.push_back(sb->getLength().getValue()); f.sb_var.push_back(sb->getLength().getVariance());
    }
    f.dg_row_begin.push_back(0);
    for (auto *g : groups_) {
        for (ObservationParameter *op : g->observations()) {
            f.dg_slot.push_back(op->getReferenceParameter()->slot);
            f.dg_obs.push_back(op->getValue());
            f.dg_var.push_back(op->getVariance());
        }
        f.dg_row_begin.push_back((int32_t)f.dg_slot.size());
        if (g->hasFullyPopulatedWeightMatrix()) {
            f.dg_disp_offset.push_back((int64_t)f.dg_disp.size());
            f.dg_disp.insert(f.dg_disp.end(), g->dispersion().begin(), g->dispersion().end());
        } else
            f.dg_disp_offset.push_back(-1);
    }
    pushValues();
}

void BundleAdjustment::pushValues() {
    flat.values.resize(flat.slot_param.size());
    for (size_t s = 0; s < flat.slot_param.size(); s++) flat.values[s] = flat.slot_param[s]->getValue();
    // observed values of directly observed groups move with the centroid (BA:180-200)
    size_t r = 0;
    for (auto *g : groups_)
        for (ObservationParameter *op : g->observations()) flat.dg_obs[r++] = op->getValue();
}

void BundleAdjustment::pullValues(const std::vector<double> &v) {
    for (size_t s = 0; s < flat.slot_param.size(); s++) flat.slot_param[s]->setValue(v[s]);
}

// ---------------------------------------------------------------------------------------------------------------
// BundleAdjustment.estimateModel (BundleAdjustment.java:203-387) with updateModel (BA:389-442): the loop stays on the
// host exactly as in the reference; BA:235 (createNormalEquation), BA:238/270-297 (precondition + MathExtension.solve)
// and BA:397/430 (getOmega) are the calls that cross the C ABI.
// ---------------------------------------------------------------------------------------------------------------
EstimationStateType BundleAdjustment::estimateModel() {
    fire("BUSY", 0, 1);
    bool deriveFirst = damping_ > 0;
    double adapted = 0.0, lastValid = 0.0;
    maxAbsDx_ = 0.0;
    int runs = maxIter_ - 1;
    bool isEstimated = false, complete = false, isConverge = true;
    if (maxIter_ == 0) { complete = isEstimated = true; adapted = 0; }
    sigma2apriori_ = sigma2apriori_ > 0 ? sigma2apriori_ : 1.0;
    try {
        prepareUnknownParameters();
        if (centroided_) centroidCoordinates(false);
        flatten();
    } catch (const std::exception &ex) {
        lastError_ = ex.what();
        return EstimationStateType::NOT_INITIALISED;
    }
    const Flat &f = flat;
    jaicov_problem_desc d;
    std::memset(&d, 0, sizeof(d));
    d.struct_size = sizeof(d);
    d.n_unknowns = numberOfUnknownParameters_ + rankDefect_.getDefect();
    d.rank_defect = rankDefect_.getDefect();
    d.datum_flags = rankDefect_.flags();
    d.n_points = (int)objectCoordinates_.size(); d.n_cameras = (int)cameras_.size(); d.n_images = (int)f.image_camera.size();
    d.n_dist = (int)f.dist_kind.size(); d.n_image_points = (int)f.ip_image.size(); d.n_image_blocks = (int)f.blk_ip_begin.size() - 1;
    d.n_scale_bars = (int)f.sb_a.size(); d.n_direct_groups = (int)f.dg_row_begin.size() - 1; d.n_direct_rows = (int)f.dg_slot.size();
    d.point_col = f.point_col.data(); d.point_datum = f.point_datum.data(); d.io_col = f.io_col.data(); d.cam_r0 = f.cam_r0.data();
    d.cam_dist_begin = f.cam_dist_begin.data(); d.dist_kind = f.dist_kind.data(); d.dist_order = f.dist_order.data(); d.dist_col = f.dist_col.data();
    d.image_camera = f.image_camera.data(); d.eo_col = f.eo_col.data(); d.ip_image = f.ip_image.data(); d.ip_point = f.ip_point.data();
    d.ip_x = f.ip_x.data(); d.ip_y = f.ip_y.data(); d.ip_var_x = f.ip_var_x.data(); d.ip_var_y = f.ip_var_y.data(); d.ip_rho = f.ip_rho.data();
    d.blk_ip_begin = f.blk_ip_begin.data(); d.blk_disp_offset = f.blk_disp_offset.data(); d.blk_disp = f.blk_disp.data();
    d.sb_point_a = f.sb_a.data(); d.sb_point_b = f.sb_b.data(); d.sb_length = f.sb_len.data(); d.sb_var = f.sb_var.data();
    d.dg_row_begin = f.dg_row_begin.data(); d.dg_slot = f.dg_slot.data(); d.dg_obs = f.dg_obs.data(); d.dg_var = f.dg_var.data();
    d.dg_disp_offset = f.dg_disp_offset.data(); d.dg_disp = f.dg_disp.data();

    jaicov_engine_options eo;
    std::memset(&eo, 0, sizeof(eo));
    eo.struct_size = sizeof(eo); eo.device = device_; eo.image_begin = eo.image_end = -1; eo.apply_shared = 1;
    int rc = jaicov_neq_create(&d, &eo, &engine_);
    auto fail = [&](int code) {
        lastError_ = engine_ ? jaicov_neq_last_error(engine_) : "engine creation failed";
        if (code == JAICOV_ERR_OUT_OF_MEMORY) return EstimationStateType::OUT_OF_MEMORY;        // BA:370-375
        if (code > 0 || code == JAICOV_ERR_BAD_ARGUMENT) return EstimationStateType::SINGULAR_MATRIX;   // BA:304-309
        return EstimationStateType::INTERRUPT;                                                     // BA:310-315
    };
    if (rc != JAICOV_OK) return fail(rc);
    if ((rc = jaicov_neq_set_parameters(engine_, f.values.data(), f.values.size())) != JAICOV_OK) return fail(rc);
    const int U = d.n_unknowns;
    const bool simulation = estimationType_ == EstimationType::SIMULATION;
    // REDUCED / PRE_ELIMINATION (BA:261-267, 283-291, 1197-1453): the final pass inverts the system from which the
    // exterior orientations were eliminated, so Qxx holds the block of the datum border, the points, the interior
    // orientation and the distortion parameters only.  The engine eliminates the EO blocks itself in every pass whenever
    // the problem allows it (jaicov_neq_reduced_order() < U), whatever the mode; where it cannot, REDUCED is served by the
    // full inverse (a superset of what the reference leaves in N).
    const bool wantInverse = inversion_ != MatrixInversion::NONE;
    const int invertMode = inversion_ == MatrixInversion::NONE ? JAICOV_INVERT_NONE
                         : inversion_ == MatrixInversion::FULL ? JAICOV_INVERT_FULL_EXPANDED : JAICOV_INVERT_REDUCED;   // FULL: all of Qxx,
    // expanded from the inverse of the EO-reduced system where the engine can pre-eliminate (jaicov_neq.h), else the plain full inverse
    std::vector<double> dx((size_t)std::max(U, 1));
    EstimationStateType status = EstimationStateType::BUSY;
    do {
        maxAbsDx_ = 0.0;
        iterationStep_ = maxIter_ - runs;
        fire("ITERATE", maxIter_, iterationStep_);
        if (deriveFirst) { adapted = damping_; deriveFirst = false; }                         // BA:801-812
        jaicov_neq_prepare_inverse(engine_, isEstimated ? invertMode : JAICOV_INVERT_NONE);   // BA:250: the final pass is known before it is built
        if ((rc = jaicov_neq_build(engine_, sigma2apriori_, adapted, simulation ? 1 : 0)) != JAICOV_OK) return fail(rc);   // BA:235
        if (interrupt_) { interrupt_ = false; return EstimationStateType::INTERRUPT; }         // BA:240-245
        complete = isEstimated;
        if (complete && wantInverse) fire("INVERT_NORMAL_EQUATION_MATRIX", 0, 1);
        if ((rc = jaicov_neq_solve(engine_, complete ? invertMode : JAICOV_INVERT_NONE, dx.data())) != JAICOV_OK) return fail(rc);     // BA:264,270,294
        // ---- updateModel (BA:389-442) ----
        bool rejected = false;
        if (adapted > 0) {
            double alpha = 0.25 * std::pow(adapted, -0.05);
            alpha = std::min(alpha, 0.75);
            for (auto &v : dx) v *= alpha;
            double prevOmega = omega_, curOmega = 0.0;
            if ((rc = jaicov_neq_omega(engine_, sigma2apriori_, dx.data(), &curOmega)) != JAICOV_OK) return fail(rc);
            prevOmega = prevOmega <= 0 ? 1.7976931348623157e308 : prevOmega;
            const bool lmaConverge = prevOmega >= curOmega;
            omega_ = curOmega;
            const double last = adapted;
            if (lmaConverge) adapted *= 0.2;
            else {
                adapted *= 5.0;
                if (adapted > 1.0 / SQRT_EPS) { adapted = 1.0 / SQRT_EPS; omega_ = 0.0; }
            }
            fire("LEVENBERG_MARQUARDT_STEP", last, adapted);
            if (!lmaConverge) { maxAbsDx_ = lastValid; rejected = true; }
        }
        if (!rejected) {
            if (complete) {
                if (simulation) omega_ = 0.0;
                else if ((rc = jaicov_neq_omega(engine_, sigma2apriori_, dx.data(), &omega_)) != JAICOV_OK) return fail(rc);
            }
            if ((rc = jaicov_neq_update(engine_, dx.data(), &maxAbsDx_)) != JAICOV_OK) return fail(rc);   // BA:450-462
            lastValid = maxAbsDx_;
        }
        if (interrupt_) { interrupt_ = false; return EstimationStateType::INTERRUPT; }
        // ---- BA:327-353 ----
        if (std::isinf(maxAbsDx_) || std::isnan(maxAbsDx_)) return EstimationStateType::SINGULAR_MATRIX;
        else if (maxAbsDx_ <= SQRT_EPS && runs > 0 && adapted == 0) {
            isEstimated = true;
            fire("CONVERGENCE", SQRT_EPS, maxAbsDx_);
        } else if (runs-- <= 1) {
            if (complete) { fire("NO_CONVERGENCE", SQRT_EPS, maxAbsDx_); isConverge = false; }
            isEstimated = true;
        } else
            fire("CONVERGENCE", SQRT_EPS, maxAbsDx_);
        if (isEstimated || adapted <= SQRT_EPS || runs < maxIter_ * 0.5 + 1) adapted = 0.0;
    } while (!complete);

    std::vector<double> v(f.values.size());
    if ((rc = jaicov_neq_get_parameters(engine_, v.data(), v.size())) != JAICOV_OK) return fail(rc);
    pullValues(v);
    Qxx_.clear();
    qxxOnDevice_ = wantInverse;      // fetched by getCofactorMatrix() / gathered by cofactorSub() on demand
    if (centroided_) centroidCoordinates(true);      // BA:357-358
    if (resultWriter_) {                             // BA:360-368, exportAdjustmentResults BA:1164-1171
        fire("EXPORT_ADJUSTMENT_RESULTS", 0.0, 0.0);
        try {
            resultWriter_->exportResults(*this);
        } catch (const std::exception &ex) {
            lastError_ = ex.what();
            fire("EXPORT_ADJUSTMENT_RESULTS_FAILED", 0.0, 1.0);
            return EstimationStateType::EXPORT_ADJUSTMENT_RESULTS_FAILED;
        }
    }
    status = isConverge ? EstimationStateType::ERROR_FREE_ESTIMATION : EstimationStateType::NO_CONVERGENCE;   // BA:377-384
    fire(isConverge ? "ERROR_FREE_ESTIMATION" : "NO_CONVERGENCE", SQRT_EPS, maxAbsDx_);
    return status;
}

void BundleAdjustment::fetchCofactor() const {
    if (!qxxOnDevice_ || !engine_) return;
    // packed 'U' (column-major upper): the leading k x k block is the leading k(k+1)/2 entries, so the reduced
    // cofactor matrix lands where the reference's in-place solve(N, n, numRows, true) leaves it (BA:264,274)
    const size_t k = (size_t)jaicov_neq_cofactor_order(engine_);
    Qxx_.assign(jaicov_neq_packed_length(engine_), 0.0);
    const int rc = jaicov_neq_get_cofactor(engine_, Qxx_.data(), k * (k + 1) / 2);
    if (rc != JAICOV_OK) { Qxx_.clear(); throw std::runtime_error(std::string("jaicov_neq_get_cofactor: ") + jaicov_neq_last_error(engine_)); }
    qxxOnDevice_ = false;
}

std::vector<double> BundleAdjustment::cofactorSub(const std::vector<int32_t> &idx, double scale) const {
    const size_t k = idx.size();
    std::vector<double> out(k * k);
    if (k == 0) return out;
    if (engine_ && (qxxOnDevice_ || !Qxx_.empty())) {
        const int rc = jaicov_neq_get_dispersion_sub(engine_, scale, idx.data(), (int32_t)k, out.data());
        if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_neq_get_dispersion_sub: ") + jaicov_neq_last_error(engine_));
        return out;
    }
    if (Qxx_.empty()) throw std::runtime_error("no cofactor matrix (MatrixInversion.NONE or not estimated)");
    for (size_t r = 0; r < k; r++)
        for (size_t c = 0; c < k; c++) {
            int a = idx[r], b = idx[c];
            if (a > b) std::swap(a, b);
            out[r * k + c] = scale * Qxx_.at((size_t)a + (size_t)b * (b + 1) / 2);
        }
    return out;
}

BundleAdjustment::ObservationReliability BundleAdjustment::observationReliability(double sigma2Test) const {
    if (!engine_ || inversion_ != MatrixInversion::FULL)
        throw std::runtime_error("no full cofactor matrix: run estimateModel with MatrixInversion.FULL first");
    int32_t n = 0;
    int rc = jaicov_rel_run(engine_, sigma2Test, nullptr, &n);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_rel_run: ") + jaicov_neq_last_error(engine_));
    ObservationReliability o;
    o.v.resize(n); o.qvv.resize(n); o.r.resize(n); o.t.resize(n);
    rc = jaicov_rel_get(engine_, o.v.data(), o.qvv.data(), o.r.data(), o.t.data(), n);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_rel_get: ") + jaicov_neq_last_error(engine_));
    return o;
}

BundleAdjustment::ImagePointReliability BundleAdjustment::imagePointReliability(double sigma2Test, double lambda0) const {
    if (!engine_ || inversion_ != MatrixInversion::FULL)
        throw std::runtime_error("no full cofactor matrix: run estimateModel with MatrixInversion.FULL first");
    int32_t rows = 0, n = 0;
    int rc = jaicov_rel_run_points(engine_, sigma2Test, nullptr, lambda0, omega_, (int32_t)getDegreeOfFreedom(), &rows, &n);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_rel_run_points: ") + jaicov_neq_last_error(engine_));
    std::vector<double> tab((size_t)JAICOV_REL_POINT_COLUMNS * (size_t)n);
    rc = jaicov_rel_get_points(engine_, tab.data(), n);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_rel_get_points: ") + jaicov_neq_last_error(engine_));
    ImagePointReliability o;
    std::vector<double> *cols[JAICOV_REL_POINT_COLUMNS] = {&o.q, &o.Tprio, &o.Tpost, &o.nablaX, &o.nablaY, &o.Mxx, &o.Mxy, &o.Myy,
                                                           &o.mdbMajor, &o.mdbMinor, &o.deltaExt, &o.dX, &o.dY, &o.dZ};
    for (int c = 0; c < JAICOV_REL_POINT_COLUMNS; c++) cols[c]->assign(tab.begin() + (size_t)c * n, tab.begin() + (size_t)(c + 1) * n);
    return o;
}

void BundleAdjustment::transformDatum() {
    if (!engine_ || inversion_ == MatrixInversion::NONE || !hasCofactorMatrix())
        throw std::runtime_error("no cofactor matrix: run estimateModel with MatrixInversion FULL or REDUCED first");
    std::vector<uint8_t> mask(objectCoordinates_.size());
    for (size_t i = 0; i < objectCoordinates_.size(); i++) mask[i] = objectCoordinates_[i]->isDatum() ? 1 : 0;
    const int rc = jaicov_datum_transform(engine_, mask.data(), (int32_t)mask.size());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_datum_transform: ") + jaicov_neq_last_error(engine_));
    Qxx_.clear();
    qxxOnDevice_ = true;      // a copy fetched before is stale: fetched again on demand
}

// include/jaicov_precision.h on the engine of the last estimateModel
static void requireCofactorOnEngine(const jaicov_engine *e, bool has) {
    if (!e || !has) throw std::runtime_error("no cofactor matrix: run estimateModel with MatrixInversion FULL or REDUCED first");
}

BundleAdjustment::PrecisionTable BundleAdjustment::pointPrecision(double sigma2, double k3, double k2, const std::vector<int32_t> &points) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    PrecisionTable t;
    t.columns = JAICOV_PREC_POINT_COLUMNS;
    const size_t n = points.empty() ? objectCoordinates_.size() : points.size();
    t.table.resize(n * t.columns);
    t.status.resize(n);
    const int rc = jaicov_prec_points(engine_, sigma2, k3, k2, points.empty() ? nullptr : points.data(), (int32_t)n, t.table.data(), t.status.data());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_prec_points: ") + jaicov_neq_last_error(engine_));
    return t;
}

BundleAdjustment::PrecisionTable BundleAdjustment::stationPrecision(double sigma2, double k3, double k2, const std::vector<int32_t> &images) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    PrecisionTable t;
    t.columns = JAICOV_PREC_STATION_COLUMNS;
    const size_t n = images.empty() ? flat.eo_col.size() / 6 : images.size();
    t.table.resize(n * t.columns);
    t.status.resize(n);
    const int rc = jaicov_prec_stations(engine_, sigma2, k3, k2, images.empty() ? nullptr : images.data(), (int32_t)n, t.table.data(), t.status.data());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_prec_stations: ") + jaicov_neq_last_error(engine_));
    return t;
}

BundleAdjustment::PrecisionTable BundleAdjustment::lengthPrecision(double sigma2, const std::vector<int32_t> &pairs) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    if (pairs.size() % 2) throw std::runtime_error("lengthPrecision: pairs must hold two point indices per length");
    PrecisionTable t;
    t.columns = JAICOV_PREC_LENGTH_COLUMNS;
    const size_t n = pairs.size() / 2;
    t.table.resize(n * t.columns);
    t.status.resize(n);
    int32_t none = 0;
    const int rc = jaicov_prec_lengths(engine_, sigma2, n ? pairs.data() : &none, (int32_t)n, t.table.data(), t.status.data());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_prec_lengths: ") + jaicov_neq_last_error(engine_));
    return t;
}

BundleAdjustment::PrincipalComponents BundleAdjustment::principalComponents(int firstCol, int nCols, int k, double tol, int maxIterations) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    PrincipalComponents c;
    const size_t kk = (size_t)std::max(k, 0), nn = (size_t)std::max(nCols, 0);
    c.values.resize(kk); c.residuals.resize(kk); c.vectors.resize(kk * nn);
    double none = 0.0;
    int32_t it = 0;
    const int rc = jaicov_prec_components(engine_, firstCol, nCols, k, tol, maxIterations, kk ? c.values.data() : &none,
                                          c.vectors.empty() ? &none : c.vectors.data(), &c.trace, kk ? c.residuals.data() : &none, &it);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_prec_components: ") + jaicov_neq_last_error(engine_));
    c.iterations = std::abs(it);
    c.converged = it > 0;
    return c;
}

// include/jaicov_parameters.h on the engine of the last estimateModel
BundleAdjustment::ParameterCorrelations BundleAdjustment::parameterCorrelations(uint32_t pairMask, uint32_t flags) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    ParameterCorrelations c;
    const int n = jaicov_neq_cofactor_order(engine_);
    c.rho.resize((size_t)std::max(n, 1)); c.partner.resize(c.rho.size()); c.status.resize(c.rho.size());
    const int rc = jaicov_par_maxima(engine_, pairMask, flags, c.rho.data(), c.partner.data(), c.status.data(), n);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_par_maxima: ") + jaicov_neq_last_error(engine_));
    c.rho.resize((size_t)std::max(n, 0)); c.partner.resize(c.rho.size()); c.status.resize(c.rho.size());
    return c;
}

BundleAdjustment::CorrelatedPairs BundleAdjustment::correlatedPairs(double threshold, uint32_t pairMask, uint32_t flags, int64_t capacity) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    CorrelatedPairs p;
    const size_t cap = (size_t)std::max<int64_t>(capacity, 0);
    p.cols.resize(2 * cap + 2); p.rho.resize(cap + 1);
    const int rc = jaicov_par_pairs(engine_, pairMask, flags, threshold, capacity, p.cols.data(), p.rho.data(), &p.count);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_par_pairs: ") + jaicov_neq_last_error(engine_));
    const size_t m = p.count > capacity ? 0 : (size_t)p.count;
    p.cols.resize(2 * m); p.rho.resize(m);
    return p;
}

std::vector<double> BundleAdjustment::correlationBlock(const std::vector<int32_t> &rowCols, const std::vector<int32_t> &colCols) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    std::vector<double> out(std::max<size_t>(rowCols.size() * colCols.size(), 1));
    int32_t none = 0;
    const int rc = jaicov_par_block(engine_, rowCols.empty() ? &none : rowCols.data(), (int32_t)rowCols.size(),
                                    colCols.empty() ? &none : colCols.data(), (int32_t)colCols.size(), out.data());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_par_block: ") + jaicov_neq_last_error(engine_));
    out.resize(rowCols.size() * colCols.size());
    return out;
}

BundleAdjustment::ParameterTests BundleAdjustment::testParameters(double sigma2, const std::vector<int32_t> &groupBegin,
                                                                  const std::vector<int32_t> &groupSlot, const std::vector<double> &x0) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    if (groupBegin.empty() || groupBegin.back() != (int32_t)groupSlot.size() || (!x0.empty() && x0.size() != groupSlot.size()))
        throw std::runtime_error("testParameters: groupBegin must end at groupSlot.size(), x0 must be empty or parallel to groupSlot");
    ParameterTests t;
    const size_t n = groupBegin.size() - 1;
    t.table.resize(std::max<size_t>(n, 1) * JAICOV_PAR_TEST_COLUMNS);
    t.status.resize(std::max<size_t>(n, 1));
    int32_t none = 0;
    const int rc = jaicov_par_tests(engine_, sigma2, groupBegin.data(), groupSlot.empty() ? &none : groupSlot.data(), x0.empty() ? nullptr : x0.data(),
                                    (int32_t)n, t.table.data(), t.status.data());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_par_tests: ") + jaicov_neq_last_error(engine_));
    t.table.resize(n * JAICOV_PAR_TEST_COLUMNS);
    t.status.resize(n);
    return t;
}

// include/jaicov_forms.h on the engine of the last estimateModel
BundleAdjustment::FormFits BundleAdjustment::fitForms(double sigma2, const std::vector<int32_t> &formType, const std::vector<int32_t> &formBegin,
                                                      const std::vector<int32_t> &formPoint, int maxIterations, double tol) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    if (formBegin.size() != formType.size() + 1 || formBegin.back() != (int32_t)formPoint.size())
        throw std::runtime_error("fitForms: formBegin must have one entry more than formType and end at formPoint.size()");
    FormFits f;
    const size_t n = formType.size(), M = formPoint.size();
    f.table.resize(std::max<size_t>(n, 1) * JAICOV_FORM_COLUMNS);
    f.qpp.resize(std::max<size_t>(n, 1) * JAICOV_FORM_QPP_COLUMNS);
    f.members.resize(std::max<size_t>(M, 1) * JAICOV_FORM_MEMBER_COLUMNS);
    f.status.resize(std::max<size_t>(n, 1));
    f.memberStatus.resize(std::max<size_t>(M, 1));
    int32_t none = 0;
    const int rc = jaicov_form_fit(engine_, sigma2, (int32_t)n, formType.empty() ? &none : formType.data(), formBegin.data(),
                                   formPoint.empty() ? &none : formPoint.data(), maxIterations, tol, f.table.data(), f.qpp.data(), f.members.data(),
                                   f.status.data(), f.memberStatus.data(), nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_form_fit: ") + jaicov_neq_last_error(engine_));
    f.table.resize(n * JAICOV_FORM_COLUMNS); f.qpp.resize(n * JAICOV_FORM_QPP_COLUMNS); f.members.resize(M * JAICOV_FORM_MEMBER_COLUMNS);
    f.status.resize(n); f.memberStatus.resize(M);
    return f;
}

// include/jaicov_surfaces.h on the engine of the last estimateModel
BundleAdjustment::FormFits BundleAdjustment::fitSurfaces(double sigma2, const std::vector<int32_t> &formType, const std::vector<int32_t> &formBegin,
                                                         const std::vector<int32_t> &formPoint, const std::vector<double> &start, int maxIterations,
                                                         double tol) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    if (formBegin.size() != formType.size() + 1 || formBegin.back() != (int32_t)formPoint.size())
        throw std::runtime_error("fitSurfaces: formBegin must have one entry more than formType and end at formPoint.size()");
    if (!start.empty() && start.size() != formType.size() * JAICOV_FORM_MAX_PARAMS)
        throw std::runtime_error("fitSurfaces: start must be empty or hold seven values per form");
    FormFits f;
    const size_t n = formType.size(), M = formPoint.size();
    f.table.resize(std::max<size_t>(n, 1) * JAICOV_FORM_COLUMNS);
    f.qpp.resize(std::max<size_t>(n, 1) * JAICOV_FORM_QPP_COLUMNS);
    f.members.resize(std::max<size_t>(M, 1) * JAICOV_FORM_MEMBER_COLUMNS);
    f.status.resize(std::max<size_t>(n, 1));
    f.memberStatus.resize(std::max<size_t>(M, 1));
    int32_t none = 0;
    const int rc = jaicov_surf_fit(engine_, sigma2, (int32_t)n, formType.empty() ? &none : formType.data(), formBegin.data(),
                                   formPoint.empty() ? &none : formPoint.data(), start.empty() ? nullptr : start.data(), maxIterations, tol,
                                   f.table.data(), f.qpp.data(), f.members.data(), f.status.data(), f.memberStatus.data(), nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_surf_fit: ") + jaicov_neq_last_error(engine_));
    f.table.resize(n * JAICOV_FORM_COLUMNS); f.qpp.resize(n * JAICOV_FORM_QPP_COLUMNS); f.members.resize(M * JAICOV_FORM_MEMBER_COLUMNS);
    f.status.resize(n); f.memberStatus.resize(M);
    return f;
}

// include/jaicov_predict.h on the engine of the last estimateModel
BundleAdjustment::ImageTable BundleAdjustment::predictImagePoints(double sigma2, const std::vector<int32_t> &images, const std::vector<int32_t> &points,
                                                                  double k2) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    if (images.size() != points.size()) throw std::runtime_error("predictImagePoints: images and points must run parallel");
    ImageTable t;
    t.columns = JAICOV_PRED_POINT_COLUMNS;
    const size_t n = images.size();
    t.table.resize(n * t.columns);
    t.status.resize(n);
    const int rc = jaicov_pred_points(engine_, sigma2, k2, images.data(), points.data(), (int32_t)n, t.table.data(), t.status.data());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_pred_points: ") + jaicov_neq_last_error(engine_));
    return t;
}

BundleAdjustment::ImageCheck BundleAdjustment::checkImagePoints(const std::vector<int32_t> &images, const std::vector<int32_t> &points,
                                                                const std::vector<double> &xy, const std::vector<double> &disp, double sigma2Post,
                                                                const std::vector<int32_t> &groupBegin) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    const size_t n = images.size(), G = groupBegin.empty() ? 0 : groupBegin.size() - 1;
    if (points.size() != n || xy.size() != 2 * n || disp.size() != 3 * n)
        throw std::runtime_error("checkImagePoints: points, xy (2 per pair) and disp (3 per pair) must run parallel to images");
    ImageCheck c;
    c.table.resize(n * JAICOV_PRED_CHECK_COLUMNS);
    c.status.resize(n);
    c.groups.resize(G * JAICOV_PRED_GROUP_COLUMNS);
    c.groupStatus.resize(G);
    const int rc = jaicov_pred_check(engine_, sigma2Post > 0.0 ? sigma2Post : sigma2apriori_, images.data(), points.data(), xy.data(), disp.data(),
                                     (int32_t)n, G ? groupBegin.data() : nullptr, (int32_t)G, c.table.data(), c.status.data(), c.groups.data(),
                                     c.groupStatus.data());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_pred_check: ") + jaicov_neq_last_error(engine_));
    return c;
}

// include/jaicov_newpoints.h on the engine of the last estimateModel
BundleAdjustment::NewPoints BundleAdjustment::intersectNewPoints(double sigma2, const std::vector<int32_t> &rayBegin, const std::vector<int32_t> &rayImage,
                                                                 const std::vector<double> &xy, const std::vector<double> &disp,
                                                                 const std::vector<double> &start, const std::vector<int32_t> &pairs,
                                                                 int maxIterations) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    const size_t n = rayBegin.empty() ? 0 : rayBegin.size() - 1, R = rayImage.size(), G = pairs.size() / 2;
    if (xy.size() != 2 * R || disp.size() != 3 * R || start.size() != 3 * n || pairs.size() % 2 || (n > 0 && (size_t)rayBegin.back() != R) ||
        (n == 0 && R > 0))
        throw std::runtime_error("intersectNewPoints: xy (2 per ray), disp (3 per ray) and start (3 per point) must fit rayBegin and rayImage");
    NewPoints r;
    r.table.resize(n * JAICOV_NEWPT_COLUMNS);
    r.status.resize(n);
    r.iterations.resize(n);
    r.rayW.resize(2 * R);
    r.lengths.resize(G * JAICOV_NEWPT_PAIR_COLUMNS);
    r.lengthStatus.resize(G);
    const int rc = jaicov_newpt_intersect(engine_, sigma2, (int32_t)n, rayBegin.data(), rayImage.data(), xy.data(), disp.data(), start.data(),
                                          maxIterations, G ? pairs.data() : nullptr, (int32_t)G, r.table.data(), r.status.data(),
                                          r.iterations.data(), r.rayW.data(), r.lengths.data(), r.lengthStatus.data());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_newpt_intersect: ") + jaicov_neq_last_error(engine_));
    return r;
}

// include/jaicov_vce.h on the engine of the last estimateModel
BundleAdjustment::VarianceComponents BundleAdjustment::varianceComponents(const VarianceGroups &g, double sigma2Test) const {
    if (!engine_ || inversion_ != MatrixInversion::FULL)
        throw std::runtime_error("no full cofactor matrix: run estimateModel with MatrixInversion.FULL first");
    const size_t nIp = flat.ip_image.size(), nSb = flat.sb_a.size(), nDg = flat.dg_row_begin.size() - 1;
    if ((!g.ip.empty() && g.ip.size() != nIp) || (!g.sb.empty() && g.sb.size() != nSb) || (!g.dg.empty() && g.dg.size() != nDg))
        throw std::runtime_error("varianceComponents: ip, sb and dg hold one group per image point, scale bar and directly observed group, or are empty");
    const int G = g.nGroups;
    int rc = jaicov_vce_run(engine_, sigma2Test > 0 ? sigma2Test : sigma2apriori_, nullptr, g.ip.empty() ? nullptr : g.ip.data(),
                            g.sb.empty() ? nullptr : g.sb.data(), g.dg.empty() ? nullptr : g.dg.data(), G, nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_vce_run: ") + jaicov_neq_last_error(engine_));
    VarianceComponents r;
    r.table.resize((size_t)JAICOV_VCE_COLUMNS * G);
    r.status.resize(G);
    rc = jaicov_vce_get(engine_, r.table.data(), r.status.data(), G);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_vce_get: ") + jaicov_neq_last_error(engine_));
    double s[5];
    rc = jaicov_vce_summary(engine_, s, 5);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_vce_summary: ") + jaicov_neq_last_error(engine_));
    r.omega = s[0]; r.sumR = s[1]; r.rowsGrouped = s[2]; r.rowsUngrouped = s[3]; r.damping = s[4];
    return r;
}

// include/jaicov_calibration.h on the engine of the last estimateModel
BundleAdjustment::CalibrationField BundleAdjustment::calibrationField(double sigma2, const std::vector<int32_t> &cameras, const std::vector<double> &xy,
                                                                      const std::vector<double> &depth, double k2, uint32_t columns,
                                                                      bool withJacobian) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    const size_t n = cameras.size();
    if (xy.size() != 2 * n || (!depth.empty() && depth.size() != n))
        throw std::runtime_error("calibrationField: xy (2 per node) and depth (1 per node, or empty) must run parallel to cameras");
    CalibrationField f;
    f.table.resize(n * JAICOV_CALIB_FIELD_COLUMNS);
    f.status.resize(n);
    if (withJacobian) f.jacobian.resize(n * 2 * JAICOV_CALIB_MAX_COLUMNS);
    const int rc = jaicov_calib_field(engine_, sigma2, k2, columns, cameras.data(), xy.data(), depth.empty() ? nullptr : depth.data(), (int32_t)n,
                                      f.table.data(), withJacobian ? f.jacobian.data() : nullptr, f.status.data());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_calib_field: ") + jaicov_neq_last_error(engine_));
    return f;
}

BundleAdjustment::CalibrationCompare BundleAdjustment::compareCalibration(int camA, int camB, const std::vector<double> &xy,
                                                                          const std::vector<double> &depth, const std::vector<double> &refValues,
                                                                          const std::vector<double> &refCov, double sigma2Post, bool relative) const {
    requireCofactorOnEngine(engine_, hasCofactorMatrix());
    const size_t n = xy.size() / 2, K = refValues.size();
    const size_t nCam = flat.io_col.size() / 3;
    if (xy.size() % 2 || (!depth.empty() && depth.size() != n)) throw std::runtime_error("compareCalibration: xy holds 2 per node, depth 1 per node or nothing");
    if (K > 0 && camB >= 0 && (size_t)camB < nCam && K != 3 + (size_t)(flat.cam_dist_begin[camB + 1] - flat.cam_dist_begin[camB]))
        throw std::runtime_error("compareCalibration: refValues holds x0, y0, c and the coefficients of camera camB");
    if (!refCov.empty() && refCov.size() != K * K) throw std::runtime_error("compareCalibration: refCov is the K x K covariance of refValues");
    CalibrationCompare c;
    c.table.resize(n * JAICOV_CALIB_COMPARE_COLUMNS);
    c.status.resize(n);
    const int rc = jaicov_calib_compare(engine_, sigma2Post > 0.0 ? sigma2Post : sigma2apriori_, camA, camB, K ? refValues.data() : nullptr,
                                        refCov.empty() ? nullptr : refCov.data(), relative ? JAICOV_CALIB_RELATIVE : 0, xy.data(),
                                        depth.empty() ? nullptr : depth.data(), (int32_t)n, c.table.data(), c.status.data(), c.summary);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_calib_compare: ") + jaicov_neq_last_error(engine_));
    return c;
}

std::vector<double> BundleAdjustment::cameraValues(int cam) const {
    const size_t nCam = flat.io_col.size() / 3, nPoints = flat.point_col.size() / 3;
    if (!engine_ || cam < 0 || (size_t)cam >= nCam) throw std::runtime_error("cameraValues: no engine, or a camera out of range");
    std::vector<double> all(jaicov_neq_num_slots(engine_));
    const int rc = jaicov_neq_get_parameters(engine_, all.data(), all.size());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_neq_get_parameters: ") + jaicov_neq_last_error(engine_));
    const size_t io = 3 * nPoints + 3 * (size_t)cam, dist = 3 * nPoints + 3 * nCam;
    std::vector<double> v(all.begin() + io, all.begin() + io + 3);
    v.insert(v.end(), all.begin() + dist + flat.cam_dist_begin[cam], all.begin() + dist + flat.cam_dist_begin[cam + 1]);
    return v;
}

BundleAdjustment::VarianceGroups BundleAdjustment::varianceGroupsByKind() const {
    VarianceGroups g;
    g.ip.assign(flat.ip_image.size(), 0);
    g.sb.assign(flat.sb_a.size(), 1);
    g.dg.assign(flat.dg_row_begin.size() - 1, 2);
    g.nGroups = 3;
    return g;
}

BundleAdjustment::VarianceGroups BundleAdjustment::varianceGroupsByImage() const {
    VarianceGroups g;
    g.ip = flat.ip_image;
    g.nGroups = (int)flat.image_camera.size();
    return g;
}

// CTEO:49-121: rows, coordinates and sigma2 J Qxx J' on the device (jaicov_xform_run), the results copied back
void CoordinateTransformationExteriorOrientation::transform(const std::vector<ObjectCoordinate *> &objectCoordinatesToTransform,
                                                            const std::vector<std::pair<Image *, std::vector<Image *>>> &imagesToAlign,
                                                            double sigma2, BundleAdjustment &adjustment) {
    jaicov_engine *e = adjustment.nativeEngine();
    if (!e) throw std::runtime_error("no cofactor matrix: run estimateModel with MatrixInversion.FULL first");
    auto &ocs = adjustment.getObjectCoordinates();
    std::vector<int32_t> points, ref, src;
    std::vector<ObjectCoordinate *> byIndex(ocs.size(), nullptr);
    for (auto *oc : objectCoordinatesToTransform) {
        if (!oc || oc->index < 0 || oc->index >= (int)ocs.size() || ocs[oc->index] != oc)
            throw std::invalid_argument("object coordinate is not part of this adjustment");
        points.push_back(oc->index);
        byIndex[oc->index] = oc;
    }
    std::vector<Image *> images;
    for (auto *c : adjustment.getCameras())
        for (auto &im : c->images()) images.push_back(im.get());
    auto imageIndex = [&](Image *im) {
        if (!im || im->index < 0 || im->index >= (int)images.size() || images[im->index] != im)
            throw std::invalid_argument("image is not part of this adjustment");
        return im->index;
    };
    for (auto &entry : imagesToAlign)
        for (Image *im : entry.second) { ref.push_back(imageIndex(entry.first)); src.push_back(imageIndex(im)); }
    int32_t n = 0;
    int rc = jaicov_xform_run(e, points.data(), (int32_t)points.size(), ref.data(), src.data(), (int32_t)ref.size(), sigma2, &n);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_xform_run: ") + jaicov_neq_last_error(e));
    std::vector<double> xyz(3 * (size_t)n), vals(jaicov_neq_num_slots(e));
    std::vector<int32_t> ids(3 * (size_t)n);
    rc = jaicov_xform_get_coordinates(e, xyz.data(), ids.data(), n);
    if (rc == JAICOV_OK) rc = jaicov_neq_get_parameters(e, vals.data(), vals.size());
    const size_t R = 3 * (size_t)n;
    std::vector<double> cov(R * (R + 1) / 2);
    if (rc == JAICOV_OK) rc = jaicov_xform_get_covariance(e, cov.data(), cov.size());
    if (rc != JAICOV_OK) throw std::runtime_error(std::string("jaicov_xform: ") + jaicov_neq_last_error(e));
    transformed_.clear();
    for (int32_t t = 0; t < n; t++) {
        ObjectCoordinate *oc = byIndex[ids[3 * t]];
        const int32_t p = ids[3 * t];
        // the engine's values may be centred (BA:115-201); the shift of the point moves the transformed point by the same amount
        const double sh[3] = {oc->getX().getValue() - vals[3 * (size_t)p], oc->getY().getValue() - vals[3 * (size_t)p + 1],
                              oc->getZ().getValue() - vals[3 * (size_t)p + 2]};
        const std::string name = oc->getName() + " " + std::to_string(images[ids[3 * t + 1]]->getId()) + " " +
                                 std::to_string(images[ids[3 * t + 2]]->getId());
        const bool same = ids[3 * t + 1] == ids[3 * t + 2];
        auto tc = std::make_unique<ObjectCoordinate>(name, same ? oc->getX().getValue() : xyz[3 * (size_t)t] + sh[0],
                                                     same ? oc->getY().getValue() : xyz[3 * (size_t)t + 1] + sh[1],
                                                     same ? oc->getZ().getValue() : xyz[3 * (size_t)t + 2] + sh[2]);
        tc->getX().setColumn(3 * t); tc->getY().setColumn(3 * t + 1); tc->getZ().setColumn(3 * t + 2);   // CTEO:154-157, 254-256
        transformed_.push_back(std::move(tc));
    }
    covariance_ = std::move(cov);
}

// ---------------------------------------------------------------------------------------------------------------
// DirectLinearTransformation (dlt/DirectLinearTransformation.java) on the device
// ---------------------------------------------------------------------------------------------------------------
DLTCoefficients::DLTCoefficients(Image *image) : image_(image) {
    static const ParameterType order[20] = {
        ParameterType::DIRECT_LINEAR_TRANSFORMATION_B11, ParameterType::DIRECT_LINEAR_TRANSFORMATION_B12,
        ParameterType::DIRECT_LINEAR_TRANSFORMATION_B13, ParameterType::DIRECT_LINEAR_TRANSFORMATION_B14,
        ParameterType::DIRECT_LINEAR_TRANSFORMATION_B21, ParameterType::DIRECT_LINEAR_TRANSFORMATION_B22,
        ParameterType::DIRECT_LINEAR_TRANSFORMATION_B23, ParameterType::DIRECT_LINEAR_TRANSFORMATION_B24,
        ParameterType::DIRECT_LINEAR_TRANSFORMATION_B31, ParameterType::DIRECT_LINEAR_TRANSFORMATION_B32,
        ParameterType::DIRECT_LINEAR_TRANSFORMATION_B33, ParameterType::PRINCIPAL_POINT_X, ParameterType::PRINCIPAL_POINT_Y,
        ParameterType::PRINCIPAL_DISTANCE, ParameterType::CAMERA_COORDINATE_X, ParameterType::CAMERA_COORDINATE_Y,
        ParameterType::CAMERA_COORDINATE_Z, ParameterType::CAMERA_OMEGA, ParameterType::CAMERA_PHI, ParameterType::CAMERA_KAPPA};
    for (ParameterType t : order) p_.emplace_back(new UnknownParameter(t, this));
}

UnknownParameter &DLTCoefficients::get(ParameterType t) {
    for (auto &q : p_)
        if (q->getParameterType() == t) return *q;
    throw std::invalid_argument("not a DLT parameter");
}

bool DirectLinearTransformation::adjust(DLTCoefficients &coefficients, const std::map<std::string, ObjectCoordinate *> &objectCoordinates,
                                        const std::vector<RestrictionType> &restrictions) {
    return adjustAll({&coefficients}, objectCoordinates, restrictions)[0];
}

std::vector<bool> DirectLinearTransformation::adjustAll(const std::vector<DLTCoefficients *> &coefficients,
                                                        const std::map<std::string, ObjectCoordinate *> &objectCoordinates,
                                                        const std::vector<RestrictionType> &restrictions) {
    const int n = (int)coefficients.size();
    std::vector<int32_t> begin(1, 0);
    std::vector<double> xy, xyz, io;
    std::vector<uint8_t> fixed;
    for (DLTCoefficients *co : coefficients) {
        Image *image = co->getReference();
        for (auto &ic : image->coordinates()) {                           // DT:78-94: the image's order, the map's coordinates
            auto it = objectCoordinates.find(ic->getObjectCoordinate()->getName());
            if (it == objectCoordinates.end()) continue;
            ObjectCoordinate *oc = it->second;
            xy.push_back(ic->getX().getValue()); xy.push_back(ic->getY().getValue());
            xyz.push_back(oc->getX().getValue()); xyz.push_back(oc->getY().getValue()); xyz.push_back(oc->getZ().getValue());
        }
        begin.push_back((int32_t)(xy.size() / 2));
        InteriorOrientation &ior = image->getReference()->getInteriorOrientation();   // DT:304-317
        UnknownParameter *p[3] = {&ior.getPrinciplePointX(), &ior.getPrinciplePointY(), &ior.getPrincipleDistance()};
        for (UnknownParameter *q : p) {
            io.push_back(q->getValue());
            fixed.push_back(q->getColumn() == COLUMN_FIXED ? 1 : 0);
        }
    }
    std::vector<int32_t> rs;
    for (RestrictionType r : restrictions) rs.push_back((int32_t)r);
    std::vector<double> out(20 * (size_t)n);
    std::vector<int32_t> status(n), solves(n);
    const int rc = jaicov_dlt_adjust(n, begin.data(), xy.data(), xyz.data(), io.data(), fixed.data(), rs.data(), (int32_t)rs.size(),
                                     maximalNumberOfIterations_, out.data(), status.data(), solves.data(), nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error("jaicov_dlt_adjust failed with status " + std::to_string(rc));
    std::vector<bool> ok(n);
    for (int g = 0; g < n; g++) {
        DLTCoefficients *co = coefficients[g];
        for (int k = 0; k < 20; k++) co->at(k)->setValue(out[20 * (size_t)g + k]);
        for (int k = 0; k < 3; k++) co->at(11 + k)->setColumn(fixed[3 * (size_t)g + k] ? COLUMN_FIXED : COLUMN_NOT_SET);
        co->status = status[g];
        co->solves = solves[g];
        ok[g] = status[g] == JAICOV_DLT_CONVERGED;
    }
    return ok;
}

void DirectLinearTransformation::applyExteriorOrientation(DLTCoefficients &coefficients, ExteriorOrientation &eo) {
    const ParameterType t[6] = {ParameterType::CAMERA_COORDINATE_X, ParameterType::CAMERA_COORDINATE_Y, ParameterType::CAMERA_COORDINATE_Z,
                                ParameterType::CAMERA_OMEGA, ParameterType::CAMERA_PHI, ParameterType::CAMERA_KAPPA};
    for (int i = 0; i < 5; i++) eo.get(t[i]).setValue(coefficients.get(t[i]).getValue());
    double kappa = coefficients.get(ParameterType::CAMERA_KAPPA).getValue();
    if (coefficients.getReference()->getReference()->getInteriorOrientation().getPrincipleDistance().getValue() < 0) {
        kappa += M_PI;                                                    // Q1: (|c|, kappa + pi) -> (c < 0, kappa)
        if (kappa > M_PI) kappa -= 2.0 * M_PI;
    }
    eo.get(ParameterType::CAMERA_KAPPA).setValue(kappa);
}

// ---------------------------------------------------------------------------------------------------------------
// ForwardIntersection (include/jaicov_intersect.h) on the device
// ---------------------------------------------------------------------------------------------------------------
std::vector<ForwardIntersection::Result> ForwardIntersection::intersectAll(const std::vector<Camera *> &cameras, double sigma2apriori,
                                                                           double rejectThreshold, int minRays) {
    struct Ray { int image; ImageCoordinate *ic; };
    std::vector<ObjectCoordinate *> points;                               // first-seen order
    std::unordered_map<ObjectCoordinate *, size_t> indexOf;
    std::vector<std::vector<Ray>> rays;
    std::vector<double> io, eo;
    int n_images = 0;
    for (Camera *cam : cameras) {
        InteriorOrientation &ior = cam->getInteriorOrientation();
        for (auto &im : cam->images()) {
            for (int k = 0; k < 3; k++) io.push_back(ior.at(k)->getValue());
            for (int k = 0; k < 6; k++) eo.push_back(im->getExteriorOrientation().at(k)->getValue());
            for (auto &ic : im->coordinates()) {
                ObjectCoordinate *oc = ic->getObjectCoordinate();
                auto it = indexOf.find(oc);
                if (it == indexOf.end()) {
                    it = indexOf.emplace(oc, points.size()).first;
                    points.push_back(oc);
                    rays.emplace_back();
                }
                rays[it->second].push_back({n_images, ic.get()});
            }
            n_images++;
        }
    }
    const int n = (int)points.size();
    std::vector<int32_t> begin(1, 0), image;
    std::vector<double> xy, var;
    for (auto &rs : rays) {
        for (const Ray &r : rs) {
            image.push_back(r.image);
            xy.push_back(r.ic->getX().getValue()); xy.push_back(r.ic->getY().getValue());
            var.push_back(r.ic->getX().getVariance()); var.push_back(r.ic->getY().getVariance());
            var.push_back(r.ic->getCorrelationCoefficientXY());
        }
        begin.push_back((int32_t)image.size());
    }
    std::vector<double> out((size_t)JAICOV_ISECT_OUT_PER_POINT * n);
    std::vector<int32_t> status(n), iterations(n);
    std::vector<uint8_t> used(image.size());
    const int rc = jaicov_isect_points(n, begin.data(), image.data(), xy.data(), var.data(), n_images, io.data(), eo.data(), sigma2apriori,
                                       maximalNumberOfIterations_, rejectThreshold, minRays, out.data(), status.data(), iterations.data(),
                                       used.data(), nullptr, nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error("jaicov_isect_points failed with status " + std::to_string(rc));
    std::vector<Result> res(n);
    for (int p = 0; p < n; p++) {
        Result &r = res[p];
        r.point = points[p];
        r.status = status[p];
        r.iterations = iterations[p];
        r.rays = begin[p + 1] - begin[p];
        for (int k = begin[p]; k < begin[p + 1]; k++) r.raysUsed += used[k];
        for (int k = 0; k < JAICOV_ISECT_OUT_PER_POINT; k++) r.values[k] = out[(size_t)JAICOV_ISECT_OUT_PER_POINT * p + k];
        if (r.status == JAICOV_ISECT_OK || r.status == JAICOV_ISECT_NOT_CONVERGED) {
            r.point->getX().setValue(r.values[0]); r.point->getY().setValue(r.values[1]); r.point->getZ().setValue(r.values[2]);
        }
    }
    return res;
}

// ---------------------------------------------------------------------------------------------------------------
// SpatialResection (include/jaicov_resect.h) on the device
// ---------------------------------------------------------------------------------------------------------------
std::vector<SpatialResection::Result> SpatialResection::resectAll(const std::vector<Camera *> &cameras, bool fromCurrentValues,
                                                                  double sigma2apriori, double rejectThreshold, int minPoints) {
    std::vector<Image *> images;
    std::vector<int32_t> begin(1, 0);
    std::vector<double> xy, xyz, var, io, eo;
    for (Camera *cam : cameras) {
        InteriorOrientation &ior = cam->getInteriorOrientation();
        for (auto &im : cam->images()) {
            images.push_back(im.get());
            for (int k = 0; k < 3; k++) io.push_back(ior.at(k)->getValue());
            for (int k = 0; k < 6; k++) eo.push_back(im->getExteriorOrientation().at(k)->getValue());
            for (auto &ic : im->coordinates()) {
                ObjectCoordinate *oc = ic->getObjectCoordinate();
                xy.push_back(ic->getX().getValue()); xy.push_back(ic->getY().getValue());
                xyz.push_back(oc->getX().getValue()); xyz.push_back(oc->getY().getValue()); xyz.push_back(oc->getZ().getValue());
                var.push_back(ic->getX().getVariance()); var.push_back(ic->getY().getVariance());
                var.push_back(ic->getCorrelationCoefficientXY());
            }
            begin.push_back((int32_t)(xy.size() / 2));
        }
    }
    const int n = (int)images.size();
    std::vector<double> out((size_t)JAICOV_RESECT_OUT_PER_IMAGE * n);
    std::vector<int32_t> status(n), iterations(n), kind(n);
    std::vector<uint8_t> used(xy.size() / 2);
    const int rc = jaicov_resect_images(n, begin.data(), xy.data(), xyz.data(), var.data(), io.data(), fromCurrentValues ? eo.data() : nullptr,
                                        sigma2apriori, maximalNumberOfIterations_, rejectThreshold, minPoints, out.data(), status.data(),
                                        iterations.data(), kind.data(), used.data(), nullptr, nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error("jaicov_resect_images failed with status " + std::to_string(rc));
    std::vector<Result> res(n);
    for (int g = 0; g < n; g++) {
        Result &r = res[g];
        r.image = images[g];
        r.status = status[g];
        r.iterations = iterations[g];
        r.startKind = kind[g];
        r.points = begin[g + 1] - begin[g];
        for (int k = begin[g]; k < begin[g + 1]; k++) r.pointsUsed += used[k];
        for (int k = 0; k < JAICOV_RESECT_OUT_PER_IMAGE; k++) r.values[k] = out[(size_t)JAICOV_RESECT_OUT_PER_IMAGE * g + k];
        if (r.status == JAICOV_RESECT_OK || r.status == JAICOV_RESECT_NOT_CONVERGED)
            for (int k = 0; k < 6; k++) r.image->getExteriorOrientation().at(k)->setValue(r.values[k]);
    }
    return res;
}

// ---------------------------------------------------------------------------------------------------------------
// RelativeOrientation (include/jaicov_relorient.h) on the device
// ---------------------------------------------------------------------------------------------------------------
namespace {
// R(omega, phi, kappa), PDF:125-135, row-major
void rotationOf(const double *a, double *R) {
    const double so = std::sin(a[0]), co = std::cos(a[0]), sp = std::sin(a[1]), cp = std::cos(a[1]), sk = std::sin(a[2]), ck = std::cos(a[2]);
    R[0] = cp * ck;                 R[1] = -cp * sk;                R[2] = sp;
    R[3] = co * sk + so * sp * ck;  R[4] = co * ck - so * sp * sk;  R[5] = -so * cp;
    R[6] = so * sk - co * sp * ck;  R[7] = so * ck + co * sp * sk;  R[8] = co * cp;
}
}  // namespace

std::vector<RelativeOrientation::Result> RelativeOrientation::orientAll(const std::vector<std::pair<Image *, Image *>> &pairs,
                                                                        bool fromCurrentValues, double sigma2apriori, double rejectThreshold,
                                                                        int minPoints) {
    std::vector<int32_t> begin(1, 0);
    std::vector<double> xa, xb, va, vb, io, start;
    for (const auto &pr : pairs) {
        std::unordered_map<ObjectCoordinate *, ImageCoordinate *> inB;
        for (auto &ic : pr.second->coordinates()) inB.emplace(ic->getObjectCoordinate(), ic.get());
        for (auto &ic : pr.first->coordinates()) {
            auto it = inB.find(ic->getObjectCoordinate());
            if (it == inB.end()) continue;
            ImageCoordinate *jc = it->second;
            xa.push_back(ic->getX().getValue()); xa.push_back(ic->getY().getValue());
            xb.push_back(jc->getX().getValue()); xb.push_back(jc->getY().getValue());
            va.push_back(ic->getX().getVariance()); va.push_back(ic->getY().getVariance()); va.push_back(ic->getCorrelationCoefficientXY());
            vb.push_back(jc->getX().getVariance()); vb.push_back(jc->getY().getVariance()); vb.push_back(jc->getCorrelationCoefficientXY());
        }
        begin.push_back((int32_t)(xa.size() / 2));
        double ea[6], eb[6], Ra[9], Rb[9];
        for (Image *im : {pr.first, pr.second})
            for (int k = 0; k < 3; k++) io.push_back(im->getReference()->getInteriorOrientation().at(k)->getValue());
        for (int k = 0; k < 6; k++) {
            ea[k] = pr.first->getExteriorOrientation().at(k)->getValue();
            eb[k] = pr.second->getExteriorOrientation().at(k)->getValue();
        }
        rotationOf(ea + 3, Ra); rotationOf(eb + 3, Rb);
        double M[9];                                                       // Ra' Rb, and Ra' (X0_b - X0_a)
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) M[3 * i + j] = Ra[i] * Rb[j] + Ra[3 + i] * Rb[3 + j] + Ra[6 + i] * Rb[6 + j];
            start.push_back(Ra[i] * (eb[0] - ea[0]) + Ra[3 + i] * (eb[1] - ea[1]) + Ra[6 + i] * (eb[2] - ea[2]));
        }
        start.push_back(std::atan2(-M[5], M[8]));
        start.push_back(std::asin(std::min(1.0, std::max(-1.0, M[2]))));
        start.push_back(std::atan2(-M[1], M[0]));
    }
    const int n = (int)pairs.size();
    std::vector<double> out((size_t)JAICOV_RELOR_OUT_PER_PAIR * n);
    std::vector<int32_t> status(n), iterations(n), kind(n);
    std::vector<uint8_t> used(xa.size() / 2);
    const int rc = jaicov_relorient_pairs(n, begin.data(), xa.data(), xb.data(), va.data(), vb.data(), io.data(),
                                          fromCurrentValues ? start.data() : nullptr, sigma2apriori, maximalNumberOfIterations_, rejectThreshold,
                                          minPoints, out.data(), status.data(), iterations.data(), kind.data(), used.data(), nullptr, nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error("jaicov_relorient_pairs failed with status " + std::to_string(rc));
    std::vector<Result> res(n);
    for (int g = 0; g < n; g++) {
        Result &r = res[g];
        r.a = pairs[g].first; r.b = pairs[g].second;
        r.status = status[g];
        r.iterations = iterations[g];
        r.startKind = kind[g];
        r.points = begin[g + 1] - begin[g];
        for (int k = begin[g]; k < begin[g + 1]; k++) r.pointsUsed += used[k];
        for (int k = 0; k < JAICOV_RELOR_OUT_PER_PAIR; k++) r.values[k] = out[(size_t)JAICOV_RELOR_OUT_PER_PAIR * g + k];
    }
    return res;
}

bool RelativeOrientation::apply(const Result &r, double baseLength) {
    if (r.status != JAICOV_RELOR_OK && r.status != JAICOV_RELOR_NOT_CONVERGED) return false;
    for (int k = 0; k < 6; k++) {
        r.a->getExteriorOrientation().at(k)->setValue(0.0);
        r.b->getExteriorOrientation().at(k)->setValue(k < 3 ? baseLength * r.values[k] : r.values[k]);
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// SimilarityTransformation (include/jaicov_simil.h) on the device
// ---------------------------------------------------------------------------------------------------------------
std::vector<SimilarityTransformation::Result> SimilarityTransformation::estimateAll(const std::vector<Model> &models, double rejectThreshold,
                                                                                    int minPoints) {
    std::vector<int32_t> begin(1, 0);
    std::vector<double> src, dst, qs, qd;
    bool withSource = false, withTarget = false;
    for (const Model &m : models) {
        withSource = withSource || !m.cofSource.empty();
        withTarget = withTarget || !m.cofTarget.empty();
    }
    for (const Model &m : models) {
        const size_t n = m.points.size();
        if (m.target.size() != n || (!m.cofSource.empty() && m.cofSource.size() != n) || (!m.cofTarget.empty() && m.cofTarget.size() != n))
            throw std::invalid_argument("SimilarityTransformation: the sizes of a model's arrays do not agree");
        for (size_t k = 0; k < n; k++) {
            src.push_back(m.points[k]->getX().getValue()); src.push_back(m.points[k]->getY().getValue()); src.push_back(m.points[k]->getZ().getValue());
            for (int i = 0; i < 3; i++) dst.push_back(m.target[k][i]);
            // a batch in which some model has cofactors gives every other model the defaults: 0 for the source, I for the target
            for (int i = 0; withSource && i < 6; i++) qs.push_back(m.cofSource.empty() ? 0.0 : m.cofSource[k][i]);
            for (int i = 0; withTarget && i < 6; i++) qd.push_back(m.cofTarget.empty() ? (i == 0 || i == 3 || i == 5 ? 1.0 : 0.0) : m.cofTarget[k][i]);
        }
        begin.push_back((int32_t)(src.size() / 3));
    }
    const int n = (int)models.size();
    std::vector<double> out((size_t)JAICOV_SIMIL_OUT_PER_MODEL * n), q(src.size() / 3);
    std::vector<int32_t> status(n), iterations(n), kind(n);
    std::vector<uint8_t> used(src.size() / 3);
    const int rc = jaicov_simil_models(n, begin.data(), src.data(), dst.data(), withSource ? qs.data() : nullptr, withTarget ? qd.data() : nullptr,
                                       nullptr, maximalNumberOfIterations_, rejectThreshold, minPoints, out.data(), status.data(),
                                       iterations.data(), kind.data(), used.data(), q.data(), nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error("jaicov_simil_models failed with status " + std::to_string(rc));
    std::vector<Result> res(n);
    for (int g = 0; g < n; g++) {
        Result &r = res[g];
        r.status = status[g];
        r.iterations = iterations[g];
        r.startKind = kind[g];
        r.points = begin[g + 1] - begin[g];
        for (int k = begin[g]; k < begin[g + 1]; k++) {
            r.pointsUsed += used[k];
            r.used.push_back(used[k] != 0);
            r.q.push_back(q[k]);
        }
        for (int k = 0; k < JAICOV_SIMIL_OUT_PER_MODEL; k++) r.values[k] = out[(size_t)JAICOV_SIMIL_OUT_PER_MODEL * g + k];
    }
    return res;
}

bool SimilarityTransformation::apply(const Result &r, const std::vector<ObjectCoordinate *> &points, const std::vector<Image *> &images) {
    if (r.status != JAICOV_SIMIL_OK && r.status != JAICOV_SIMIL_NOT_CONVERGED) return false;
    const int32_t pb[2] = {0, (int32_t)points.size()}, ib[2] = {0, (int32_t)images.size()};
    std::vector<double> xyz, eo;
    for (ObjectCoordinate *p : points) {
        xyz.push_back(p->getX().getValue()); xyz.push_back(p->getY().getValue()); xyz.push_back(p->getZ().getValue());
    }
    for (Image *im : images)
        for (int k = 0; k < 6; k++) eo.push_back(im->getExteriorOrientation().at(k)->getValue());
    const int rc = jaicov_simil_apply(1, r.values, points.empty() ? nullptr : pb, xyz.data(), nullptr, images.empty() ? nullptr : ib, eo.data(),
                                      xyz.data(), nullptr, eo.data());
    if (rc != JAICOV_OK) throw std::runtime_error("jaicov_simil_apply failed with status " + std::to_string(rc));
    for (size_t k = 0; k < points.size(); k++) {
        points[k]->getX().setValue(xyz[3 * k]); points[k]->getY().setValue(xyz[3 * k + 1]); points[k]->getZ().setValue(xyz[3 * k + 2]);
    }
    for (size_t g = 0; g < images.size(); g++)
        for (int k = 0; k < 6; k++) images[g]->getExteriorOrientation().at(k)->setValue(eo[6 * g + k]);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// LensCorrection (include/jaicov_lens.h) on the device
// ---------------------------------------------------------------------------------------------------------------
std::vector<LensCorrection::Result> LensCorrection::run(Camera &camera, bool correct, bool withDistance, double tolerance) {
    // the camera's tables, as flatten() lays them out
    InteriorOrientation &io = camera.getInteriorOrientation();
    const double cam_io[3] = {io.getPrinciplePointX().getValue(), io.getPrinciplePointY().getValue(), io.getPrincipleDistance().getValue()};
    double r0 = 0.0;
    std::vector<int32_t> kind, order;
    std::vector<double> value;
    for (auto &m : camera.getDistortionModels()) {
        if (m->getType() >= DistortionModel::Type::RADIAL_DISTORTION) r0 = m->getR0();
        if (m->getType() == DistortionModel::Type::DISTANCE_DISTORTION && !withDistance) continue;
        for (auto &p : m->parameters()) {
            int k;
            switch (p->getParameterType()) {
            case ParameterType::AFFINITY_AND_SHEAR_Cx: k = JAICOV_DIST_AFFINITY_CX; break;
            case ParameterType::AFFINITY_AND_SHEAR_Cy: k = JAICOV_DIST_AFFINITY_CY; break;
            case ParameterType::TANGENTIAL_DISTORTION_Bx: k = JAICOV_DIST_TANGENTIAL_BX; break;
            case ParameterType::TANGENTIAL_DISTORTION_By: k = JAICOV_DIST_TANGENTIAL_BY; break;
            case ParameterType::TANGENTIAL_POLYNOMIAL_B: k = JAICOV_DIST_TANGENTIAL_BI; break;
            case ParameterType::RADIAL_POLYNOMIAL_A: k = JAICOV_DIST_RADIAL_AI; break;
            case ParameterType::ZERNIKE_POLYNOMIAL_X: k = JAICOV_DIST_ZERNIKE_X; break;
            case ParameterType::ZERNIKE_POLYNOMIAL_Y: k = JAICOV_DIST_ZERNIKE_Y; break;
            case ParameterType::ZERNIKE_POLYNOMIAL_Z: k = JAICOV_DIST_ZERNIKE_Z; break;
            default: k = JAICOV_DIST_DISTANCE_DI; break;
            }
            kind.push_back(k); order.push_back(p->getOrder() > 0 ? p->getOrder() : 0); value.push_back(p->getValue());
        }
    }
    const int32_t begin[2] = {0, (int32_t)kind.size()};
    std::vector<Result> res;
    std::vector<double> xy, var, depth;
    for (auto &im : camera.images()) {
        ExteriorOrientation &eo = im->getExteriorOrientation();
        const double so = std::sin(eo.at(3)->getValue()), co = std::cos(eo.at(3)->getValue());
        const double sp = std::sin(eo.at(4)->getValue()), cp = std::cos(eo.at(4)->getValue());
        for (auto &ic : im->coordinates()) {
            Result r;
            r.coordinate = ic.get();
            res.push_back(r);
            xy.push_back(ic->getX().getValue()); xy.push_back(ic->getY().getValue());
            var.push_back(ic->getX().getVariance()); var.push_back(ic->getY().getVariance()); var.push_back(ic->getCorrelationCoefficientXY());
            if (withDistance) {                       // N = r13 dX + r23 dY + r33 dZ (PDF:127-135, 151)
                ObjectCoordinate *oc = ic->getObjectCoordinate();
                if (!oc) throw std::invalid_argument("LensCorrection: an image coordinate without its object coordinate has no distance");
                const double dX = oc->getX().getValue() - eo.at(0)->getValue(), dY = oc->getY().getValue() - eo.at(1)->getValue(),
                             dZ = oc->getZ().getValue() - eo.at(2)->getValue();
                depth.push_back(sp * dX + (-so * cp) * dY + (co * cp) * dZ);
            }
        }
    }
    const int n = (int)res.size();
    std::vector<int32_t> cam((size_t)n, 0), status((size_t)n), iterations((size_t)n, 0);
    std::vector<double> xyo(2 * (size_t)n), varo(3 * (size_t)n);
    const int rc = correct ? jaicov_lens_correct(n, cam.data(), xy.data(), var.data(), withDistance ? depth.data() : nullptr, 1, cam_io, &r0, begin,
                                                 kind.data(), order.data(), value.data(), maximalNumberOfIterations_, tolerance, xyo.data(),
                                                 varo.data(), nullptr, status.data(), iterations.data(), nullptr)
                           : jaicov_lens_distort(n, cam.data(), xy.data(), var.data(), withDistance ? depth.data() : nullptr, 1, cam_io, &r0, begin,
                                                 kind.data(), order.data(), value.data(), xyo.data(), varo.data(), nullptr, status.data(), nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error(std::string(correct ? "jaicov_lens_correct" : "jaicov_lens_distort") + " failed with status " + std::to_string(rc));
    for (int k = 0; k < n; k++) {
        Result &r = res[k];
        r.x = xyo[2 * k]; r.y = xyo[2 * k + 1];
        r.varianceX = varo[3 * k]; r.varianceY = varo[3 * k + 1]; r.rho = varo[3 * k + 2];
        r.status = status[k]; r.iterations = iterations[k];
    }
    return res;
}

std::vector<LensCorrection::Result> LensCorrection::correctAll(Camera &camera, bool withDistance, double tolerance) {
    return run(camera, true, withDistance, tolerance);
}

std::vector<LensCorrection::Result> LensCorrection::distortAll(Camera &camera, bool withDistance) { return run(camera, false, withDistance, 0.0); }

LensCorrection::Scope::Scope(const std::vector<Result> &results) {
    for (const Result &r : results) {
        if (!r.coordinate || (r.status != JAICOV_LENS_OK && r.status != JAICOV_LENS_NOT_CONVERGED)) continue;
        ImageCoordinate *ic = r.coordinate;
        Result old = r;
        old.x = ic->getX().getValue(); old.y = ic->getY().getValue();
        old.varianceX = ic->getX().getVariance(); old.varianceY = ic->getY().getVariance(); old.rho = ic->getCorrelationCoefficientXY();
        saved_.push_back(old);
        try {
            ic->getX().setValue(r.x); ic->getY().setValue(r.y);
            ic->getX().setVariance(r.varianceX); ic->getY().setVariance(r.varianceY); ic->setCorrelationCoefficientXY(r.rho);
        } catch (...) {                               // a setter refused a value: no destructor will run, so everything goes back here
            restore();
            throw;
        }
    }
}

void LensCorrection::Scope::restore() {
    for (auto o = saved_.rbegin(); o != saved_.rend(); ++o) {
        ImageCoordinate *ic = o->coordinate;
        ic->getX().setValue(o->x); ic->getY().setValue(o->y);
        ic->getX().setVariance(o->varianceX); ic->getY().setVariance(o->varianceY); ic->setCorrelationCoefficientXY(o->rho);
    }
    saved_.clear();
}

LensCorrection::Scope::~Scope() { restore(); }

}  // namespace jaicov::host
