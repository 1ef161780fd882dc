// jaicov.hpp -- C++17 mirror of JAICOV's object API for the bundle-adjustment path, on top of the C ABI
// (include/jaicov_neq.h).  The reference is Java (no JDK in this image), so the host side of the boundary is written in
// C++ with the reference's class / method names, argument meaning and error behaviour:
//
//   org.applied_geodesy.adjustment.bundle.{Camera, Image, ImageCoordinate, ObjectCoordinate, ScaleBar,
//       BundleAdjustment, parameter.*, camera.distortion.*, camera.orientation.*}, adjustment.defect.RankDefect,
//       adjustment.{EstimationStateType, EstimationType}
//
// What stays on the host (integer / control work, bit-exact with the reference):
//   prepareUnknownParameters  BundleAdjustment.java:667-782     detectRankDefect  BundleAdjustment.java:836-1042
//   centroidCoordinates       BundleAdjustment.java:115-201     estimateModel loop BundleAdjustment.java:203-387
//   updateModel (LM control)  BundleAdjustment.java:389-442
// What goes to the MI355X through the C ABI: createNormalEquation, applyPrecondition, MathExtension.solve, getOmega.
#pragma once
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/jaicov_neq.h"
#include "../../include/jaicov_transform.h"
#include "../../include/jaicov_dlt.h"
#include "../../include/jaicov_intersect.h"
#include "../../include/jaicov_resect.h"
#include "../../include/jaicov_relorient.h"
#include "../../include/jaicov_simil.h"
#include "../../include/jaicov_lens.h"
#include "../../include/jaicov_reliability.h"
#include "../../include/jaicov_reliability_points.h"
#include "../../include/jaicov_datum.h"
#include "../../include/jaicov_precision.h"
#include "../../include/jaicov_parameters.h"
#include "../../include/jaicov_forms.h"
#include "../../include/jaicov_surfaces.h"
#include "../../include/jaicov_predict.h"
#include "../../include/jaicov_newpoints.h"
#include "../../include/jaicov_vce.h"
#include "../../include/jaicov_calibration.h"

namespace jaicov::host {

// parameter/ParameterType.java:27-100 (ids kept)
enum class ParameterType : int {
    PRINCIPAL_POINT_X = 111, PRINCIPAL_POINT_Y = 112, PRINCIPAL_DISTANCE = 113, RADIAL_POLYNOMIAL_A = 121,
    TANGENTIAL_POLYNOMIAL_B = 131, TANGENTIAL_DISTORTION_Bx = 132, TANGENTIAL_DISTORTION_By = 133,
    AFFINITY_AND_SHEAR_Cx = 141, AFFINITY_AND_SHEAR_Cy = 142, DISTANCE_POLYNOMIAL_D = 151,
    ZERNIKE_POLYNOMIAL_X = 161, ZERNIKE_POLYNOMIAL_Y = 162, ZERNIKE_POLYNOMIAL_Z = 163,
    CAMERA_COORDINATE_X = 251, CAMERA_COORDINATE_Y = 252, CAMERA_COORDINATE_Z = 253,
    CAMERA_OMEGA = 261, CAMERA_PHI = 262, CAMERA_KAPPA = 263,
    OBJECT_COORDINATE_X = 311, OBJECT_COORDINATE_Y = 312, OBJECT_COORDINATE_Z = 313,
    IMAGE_COORDINATE_X = 411, IMAGE_COORDINATE_Y = 412, SCALE_BAR_LENGTH = 511,
    DIRECT_LINEAR_TRANSFORMATION_B11 = 611, DIRECT_LINEAR_TRANSFORMATION_B12 = 612, DIRECT_LINEAR_TRANSFORMATION_B13 = 613,
    DIRECT_LINEAR_TRANSFORMATION_B14 = 614, DIRECT_LINEAR_TRANSFORMATION_B21 = 621, DIRECT_LINEAR_TRANSFORMATION_B22 = 622,
    DIRECT_LINEAR_TRANSFORMATION_B23 = 623, DIRECT_LINEAR_TRANSFORMATION_B24 = 624, DIRECT_LINEAR_TRANSFORMATION_B31 = 631,
    DIRECT_LINEAR_TRANSFORMATION_B32 = 632, DIRECT_LINEAR_TRANSFORMATION_B33 = 633
};

inline const char *parameterTypeName(ParameterType t) {   // ParameterType.name()
    switch (t) {
    case ParameterType::PRINCIPAL_POINT_X: return "PRINCIPAL_POINT_X";
    case ParameterType::PRINCIPAL_POINT_Y: return "PRINCIPAL_POINT_Y";
    case ParameterType::PRINCIPAL_DISTANCE: return "PRINCIPAL_DISTANCE";
    case ParameterType::RADIAL_POLYNOMIAL_A: return "RADIAL_POLYNOMIAL_A";
    case ParameterType::TANGENTIAL_POLYNOMIAL_B: return "TANGENTIAL_POLYNOMIAL_B";
    case ParameterType::TANGENTIAL_DISTORTION_Bx: return "TANGENTIAL_DISTORTION_Bx";
    case ParameterType::TANGENTIAL_DISTORTION_By: return "TANGENTIAL_DISTORTION_By";
    case ParameterType::AFFINITY_AND_SHEAR_Cx: return "AFFINITY_AND_SHEAR_Cx";
    case ParameterType::AFFINITY_AND_SHEAR_Cy: return "AFFINITY_AND_SHEAR_Cy";
    case ParameterType::DISTANCE_POLYNOMIAL_D: return "DISTANCE_POLYNOMIAL_D";
    case ParameterType::ZERNIKE_POLYNOMIAL_X: return "ZERNIKE_POLYNOMIAL_X";
    case ParameterType::ZERNIKE_POLYNOMIAL_Y: return "ZERNIKE_POLYNOMIAL_Y";
    case ParameterType::ZERNIKE_POLYNOMIAL_Z: return "ZERNIKE_POLYNOMIAL_Z";
    case ParameterType::CAMERA_COORDINATE_X: return "CAMERA_COORDINATE_X";
    case ParameterType::CAMERA_COORDINATE_Y: return "CAMERA_COORDINATE_Y";
    case ParameterType::CAMERA_COORDINATE_Z: return "CAMERA_COORDINATE_Z";
    case ParameterType::CAMERA_OMEGA: return "CAMERA_OMEGA";
    case ParameterType::CAMERA_PHI: return "CAMERA_PHI";
    case ParameterType::CAMERA_KAPPA: return "CAMERA_KAPPA";
    case ParameterType::OBJECT_COORDINATE_X: return "OBJECT_COORDINATE_X";
    case ParameterType::OBJECT_COORDINATE_Y: return "OBJECT_COORDINATE_Y";
    case ParameterType::OBJECT_COORDINATE_Z: return "OBJECT_COORDINATE_Z";
    case ParameterType::IMAGE_COORDINATE_X: return "IMAGE_COORDINATE_X";
    case ParameterType::IMAGE_COORDINATE_Y: return "IMAGE_COORDINATE_Y";
    case ParameterType::SCALE_BAR_LENGTH: return "SCALE_BAR_LENGTH";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B11: return "DIRECT_LINEAR_TRANSFORMATION_B11";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B12: return "DIRECT_LINEAR_TRANSFORMATION_B12";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B13: return "DIRECT_LINEAR_TRANSFORMATION_B13";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B14: return "DIRECT_LINEAR_TRANSFORMATION_B14";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B21: return "DIRECT_LINEAR_TRANSFORMATION_B21";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B22: return "DIRECT_LINEAR_TRANSFORMATION_B22";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B23: return "DIRECT_LINEAR_TRANSFORMATION_B23";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B24: return "DIRECT_LINEAR_TRANSFORMATION_B24";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B31: return "DIRECT_LINEAR_TRANSFORMATION_B31";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B32: return "DIRECT_LINEAR_TRANSFORMATION_B32";
    case ParameterType::DIRECT_LINEAR_TRANSFORMATION_B33: return "DIRECT_LINEAR_TRANSFORMATION_B33";
    }
    return "?";
}

// adjustment/EstimationStateType.java:25-42
enum class EstimationStateType : int {
    ERROR_FREE_ESTIMATION = 1, BUSY = 0, INTERRUPT = -1, SINGULAR_MATRIX = -2, ROBUST_ESTIMATION_FAILED = -3,
    NO_CONVERGENCE = -4, NOT_INITIALISED = -5, EXPORT_ADJUSTMENT_RESULTS_FAILED = -6, OUT_OF_MEMORY = -7
};
enum class EstimationType { L2NORM, SIMULATION };                       // adjustment/EstimationType.java
enum class MatrixInversion { NONE, FULL, PRE_ELIMINATION, REDUCED };    // BundleAdjustment.java:65-70

constexpr int COLUMN_NOT_SET = -1;          // UnknownParameter.java:28
constexpr int COLUMN_FIXED = INT_MAX;       // UnknownParameter.java:27 (Integer.MAX_VALUE)

class ObjectCoordinate;
class Image;
class Camera;

// parameter/UnknownParameter.java (+ PolynomialCoefficient.order)
class UnknownParameter {
public:
    UnknownParameter(ParameterType t, void *ref, int order = -1) : type_(t), ref_(ref), order_(order) {}
    ParameterType getParameterType() const { return type_; }
    double getValue() const { return value_; }
    void setValue(double v) { value_ = v; }
    int getColumn() const { return column_; }
    void setColumn(int c) { column_ = c; }
    int getOrder() const { return order_; }
    void *getReference() const { return ref_; }
    int slot = -1;      // flattening: index into the engine's value vector
private:
    ParameterType type_;
    void *ref_;
    int order_;
    double value_ = 0.0;
    int column_ = COLUMN_NOT_SET;
};

// parameter/ObservationParameter.java
class ObservationParameter {
public:
    ObservationParameter(ParameterType t, void *ref) : type_(t), ref_(ref) {}
    explicit ObservationParameter(UnknownParameter *p) : type_(p->getParameterType()), ref_(p), unknown_(p) { value_ = p->getValue(); }
    ParameterType getParameterType() const { return type_; }
    double getValue() const { return value_; }
    void setValue(double v) { value_ = v; }
    double getVariance() const { return variance_; }
    void setVariance(double v) {
        if (!(v > 0)) throw std::invalid_argument("Error, variance must be positive");   // ObservationParameter.java:55-57
        variance_ = v;
    }
    int getRow() const { return row_; }
    void setRow(int r) { row_ = r; }
    UnknownParameter *getReferenceParameter() const { return unknown_; }
private:
    ParameterType type_;
    void *ref_;
    UnknownParameter *unknown_ = nullptr;
    double value_ = 0.0, variance_ = 0.0;
    int row_ = -1;
};

// ObjectCoordinate.java
class ObjectCoordinate {
public:
    ObjectCoordinate(const ObjectCoordinate &) = delete;
    ObjectCoordinate &operator=(const ObjectCoordinate &) = delete;
    ObjectCoordinate(std::string name, double x, double y, double z)
        : name_(std::move(name)), x_(ParameterType::OBJECT_COORDINATE_X, this), y_(ParameterType::OBJECT_COORDINATE_Y, this),
          z_(ParameterType::OBJECT_COORDINATE_Z, this) {
        x_.setValue(x); y_.setValue(y); z_.setValue(z);
    }
    const std::string &getName() const { return name_; }
    UnknownParameter &getX() { return x_; }
    UnknownParameter &getY() { return y_; }
    UnknownParameter &getZ() { return z_; }
    bool isDatum() const { return datum_; }
    void setDatum(bool d) { datum_ = d; }
    int numberOfImages() const { return n_images_; }
    void addImage() { n_images_++; }
    int index = -1;     // flattening
private:
    std::string name_;
    bool datum_ = true;
    UnknownParameter x_, y_, z_;
    int n_images_ = 0;
};

// ScaleBar.java
class ScaleBar {
public:
    ScaleBar(const ScaleBar &) = delete;
    ScaleBar &operator=(const ScaleBar &) = delete;
    ScaleBar(ObjectCoordinate *a, ObjectCoordinate *b, double value, double sigma)
        : a_(a), b_(b), length_(ParameterType::SCALE_BAR_LENGTH, this) {
        length_.setValue(value);
        length_.setVariance(sigma * sigma);
    }
    ObservationParameter &getLength() { return length_; }
    ObjectCoordinate *getObjectCoordinateA() const { return a_; }
    ObjectCoordinate *getObjectCoordinateB() const { return b_; }
private:
    ObjectCoordinate *a_, *b_;
    ObservationParameter length_;
};

// camera/distortion/DistortionModel.java:29-37
class DistortionModel {
public:
    DistortionModel(const DistortionModel &) = delete;
    DistortionModel &operator=(const DistortionModel &) = delete;
    // DistortionModel.java:29-37 (ordinal = application order, Camera.java:50)
    enum class Type { AFFINITY_AND_SHEAR = 0, TANGENTIAL_DISTORTION = 1, RADIAL_DISTORTION = 2, DISTANCE_DISTORTION = 3,
                      ZERNIKE_X = 4, ZERNIKE_Y = 5, ZERNIKE_GRADIENT = 6 };
    DistortionModel(Type t, double r0) : type_(t), r0_(r0) {
        if (t == Type::AFFINITY_AND_SHEAR) {          // AffinityShearDistortionModel.java:34-40: Cx, Cy fixed by default
            params_.emplace_back(new UnknownParameter(ParameterType::AFFINITY_AND_SHEAR_Cx, this));
            params_.emplace_back(new UnknownParameter(ParameterType::AFFINITY_AND_SHEAR_Cy, this));
            params_[0]->setColumn(COLUMN_FIXED); params_[1]->setColumn(COLUMN_FIXED);
        } else if (t == Type::TANGENTIAL_DISTORTION) { // TangentialDistortionModel.java:34-42: Bx, By fixed by default
            params_.emplace_back(new UnknownParameter(ParameterType::TANGENTIAL_DISTORTION_Bx, this));
            params_.emplace_back(new UnknownParameter(ParameterType::TANGENTIAL_DISTORTION_By, this));
            params_[0]->setColumn(COLUMN_FIXED); params_[1]->setColumn(COLUMN_FIXED);
        }
    }
    Type getType() const { return type_; }
    double getR0() const { return r0_; }
    // PolynomialDistortionModel.add(order): insertion order is iteration order (LinkedHashMap, PolynomialDistortionModel.java:34,60-62)
    UnknownParameter *add(int order) {
        if (type_ == Type::AFFINITY_AND_SHEAR) throw std::invalid_argument("affinity model has no polynomial coefficients");
        if (order <= 0) throw std::invalid_argument("Error, polynomial coefficient order must be a real positive integer.");
        for (auto &p : params_)
            if (p->getOrder() == order) throw std::invalid_argument("Error, polynomial coefficient order already exists.");
        ParameterType pt = type_ == Type::TANGENTIAL_DISTORTION ? ParameterType::TANGENTIAL_POLYNOMIAL_B
                           : type_ == Type::RADIAL_DISTORTION   ? ParameterType::RADIAL_POLYNOMIAL_A
                           : type_ == Type::DISTANCE_DISTORTION ? ParameterType::DISTANCE_POLYNOMIAL_D
                           : type_ == Type::ZERNIKE_X           ? ParameterType::ZERNIKE_POLYNOMIAL_X      // ZernikeDistortionModel.java:36-38
                           : type_ == Type::ZERNIKE_Y           ? ParameterType::ZERNIKE_POLYNOMIAL_Y      // :47-49
                                                                : ParameterType::ZERNIKE_POLYNOMIAL_Z;     // :58-60
        params_.emplace_back(new UnknownParameter(pt, this, order));
        return params_.back().get();
    }
    UnknownParameter *get(int order) {
        for (auto &p : params_)
            if (p->getOrder() == order) return p.get();
        return nullptr;
    }
    UnknownParameter *getCx() { return type_ == Type::AFFINITY_AND_SHEAR ? params_[0].get() : nullptr; }
    UnknownParameter *getCy() { return type_ == Type::AFFINITY_AND_SHEAR ? params_[1].get() : nullptr; }
    UnknownParameter *getBx() { return type_ == Type::TANGENTIAL_DISTORTION ? params_[0].get() : nullptr; }
    UnknownParameter *getBy() { return type_ == Type::TANGENTIAL_DISTORTION ? params_[1].get() : nullptr; }
    std::vector<std::unique_ptr<UnknownParameter>> &parameters() { return params_; }
private:
    Type type_;
    double r0_;
    std::vector<std::unique_ptr<UnknownParameter>> params_;
};

// camera/orientation/InteriorOrientation.java:60-82 (iteration order x0, y0, c)
class InteriorOrientation {
public:
    InteriorOrientation(const InteriorOrientation &) = delete;
    InteriorOrientation &operator=(const InteriorOrientation &) = delete;
    InteriorOrientation()
        : x0_(ParameterType::PRINCIPAL_POINT_X, this), y0_(ParameterType::PRINCIPAL_POINT_Y, this), c_(ParameterType::PRINCIPAL_DISTANCE, this) {}
    UnknownParameter &getPrinciplePointX() { return x0_; }
    UnknownParameter &getPrinciplePointY() { return y0_; }
    UnknownParameter &getPrincipleDistance() { return c_; }
    UnknownParameter *at(int i) { return i == 0 ? &x0_ : (i == 1 ? &y0_ : &c_); }
private:
    UnknownParameter x0_, y0_, c_;
};

// camera/orientation/ExteriorOrientation.java:37-46 (X0, Y0, Z0, omega, phi, kappa)
class ExteriorOrientation {
public:
    ExteriorOrientation(const ExteriorOrientation &) = delete;
    ExteriorOrientation &operator=(const ExteriorOrientation &) = delete;
    ExteriorOrientation()
        : p_{UnknownParameter(ParameterType::CAMERA_COORDINATE_X, this), UnknownParameter(ParameterType::CAMERA_COORDINATE_Y, this),
             UnknownParameter(ParameterType::CAMERA_COORDINATE_Z, this), UnknownParameter(ParameterType::CAMERA_OMEGA, this),
             UnknownParameter(ParameterType::CAMERA_PHI, this), UnknownParameter(ParameterType::CAMERA_KAPPA, this)} {}
    UnknownParameter &get(ParameterType t) {
        for (auto &q : p_)
            if (q.getParameterType() == t) return q;
        throw std::invalid_argument("not an exterior orientation parameter");
    }
    UnknownParameter *at(int i) { return &p_[i]; }
private:
    UnknownParameter p_[6];
};

// camera/ImageCoordinate.java
class ImageCoordinate {
public:
    ImageCoordinate(const ImageCoordinate &) = delete;
    ImageCoordinate &operator=(const ImageCoordinate &) = delete;
    ImageCoordinate(ObjectCoordinate *oc, Image *img, double xp, double yp, double sx, double sy, double rho)
        : oc_(oc), img_(img), rho_(rho), x_(ParameterType::IMAGE_COORDINATE_X, this), y_(ParameterType::IMAGE_COORDINATE_Y, this) {
        if (std::fabs(rho) >= 1) throw std::invalid_argument("Error, correlation coefficient rho(x,y) must be in the open interval (-1 1)");
        x_.setValue(xp); y_.setValue(yp);
        x_.setVariance(sx * sx); y_.setVariance(sy * sy);
    }
    ObjectCoordinate *getObjectCoordinate() const { return oc_; }
    ObservationParameter &getX() { return x_; }
    ObservationParameter &getY() { return y_; }
    double getCorrelationCoefficientXY() const { return rho_; }
    void setCorrelationCoefficientXY(double rho) {
        if (!(std::fabs(rho) < 1)) throw std::invalid_argument("Error, correlation coefficient rho(x,y) must be in the open interval (-1 1)");
        rho_ = rho;
    }
    Image *getReference() const { return img_; }
private:
    ObjectCoordinate *oc_;
    Image *img_;
    double rho_;
    ObservationParameter x_, y_;
};

// camera/Image.java (LinkedHashMap<ObjectCoordinate, ImageCoordinate>: insertion order, one observation per point)
class Image {
public:
    Image(const Image &) = delete;
    Image &operator=(const Image &) = delete;
    Image(long id, Camera *cam) : id_(id), cam_(cam) {}
    long getId() const { return id_; }
    Camera *getReference() const { return cam_; }
    ExteriorOrientation &getExteriorOrientation() { return eo_; }
    ImageCoordinate *add(ObjectCoordinate *oc, double xp, double yp, double sx, double sy, double rho = 0.0) {
        auto it = index_.find(oc);
        if (it != index_.end()) return coords_[it->second].get();       // Image.java:53-54
        coords_.emplace_back(new ImageCoordinate(oc, this, xp, yp, sx, sy, rho));
        index_[oc] = coords_.size() - 1;
        oc->addImage();
        return coords_.back().get();
    }
    int getNumberOfImageCoordinates() const { return (int)coords_.size(); }
    std::vector<std::unique_ptr<ImageCoordinate>> &coordinates() { return coords_; }
    // Joint, fully populated dispersion of ALL image coordinates of this image, rows x0,y0,x1,y1,... in insertion order
    // (the largest W the a10 contract can express; new relative to the reference).  Row-major (2m x 2m).
    void setDispersion(std::vector<double> D) {
        const size_t m = 2 * coords_.size();
        if (D.size() != m * m) throw std::invalid_argument("Error, number of observations and number of rows/columns in dispersion matrix are unequal");
        for (size_t i = 0; i < coords_.size(); i++) {                   // DOPG:53-55: variances from the diagonal
            coords_[i]->getX().setVariance(D[(2 * i) * m + 2 * i]);
            coords_[i]->getY().setVariance(D[(2 * i + 1) * m + 2 * i + 1]);
        }
        disp_ = std::move(D);
    }
    const std::vector<double> &dispersion() const { return disp_; }
    int index = -1;
private:
    long id_;
    Camera *cam_;
    ExteriorOrientation eo_;
    std::vector<std::unique_ptr<ImageCoordinate>> coords_;
    std::unordered_map<ObjectCoordinate *, size_t> index_;
    std::vector<double> disp_;
};

// camera/Camera.java:45-83: distortion models sorted by Type ordinal, images in insertion order
class Camera {
public:
    Camera(const Camera &) = delete;
    Camera &operator=(const Camera &) = delete;
    Camera(long id, double r0, std::vector<DistortionModel::Type> types) : id_(id) {
        std::sort(types.begin(), types.end());
        for (size_t i = 0; i < types.size(); i++) {
            if (i > 0 && types[i] == types[i - 1]) throw std::invalid_argument("Error, duplicate type of distortion model detected.");
            models_.emplace_back(new DistortionModel(types[i], r0));
        }
    }
    long getId() const { return id_; }
    InteriorOrientation &getInteriorOrientation() { return io_; }
    Image *add(long imageId) {
        auto it = index_.find(imageId);
        if (it != index_.end()) return images_[it->second].get();
        images_.emplace_back(new Image(imageId, this));
        index_[imageId] = images_.size() - 1;
        return images_.back().get();
    }
    int getNumberOfImages() const { return (int)images_.size(); }
    DistortionModel *getDistortionModel(DistortionModel::Type t) {
        for (auto &m : models_)
            if (m->getType() == t) return m.get();
        return nullptr;
    }
    std::vector<std::unique_ptr<DistortionModel>> &getDistortionModels() { return models_; }
    std::vector<std::unique_ptr<Image>> &images() { return images_; }
    int index = -1;
private:
    long id_;
    InteriorOrientation io_;
    std::vector<std::unique_ptr<DistortionModel>> models_;
    std::vector<std::unique_ptr<Image>> images_;
    std::unordered_map<long, size_t> index_;
};

// parameter/DirectlyObservedParameterGroup.java
class DirectlyObservedParameterGroup {
public:
    DirectlyObservedParameterGroup(const DirectlyObservedParameterGroup &) = delete;
    DirectlyObservedParameterGroup &operator=(const DirectlyObservedParameterGroup &) = delete;
    explicit DirectlyObservedParameterGroup(std::vector<ObservationParameter *> obs) : obs_(std::move(obs)) {
        std::unordered_set<ObservationParameter *> u(obs_.begin(), obs_.end());
        if (u.size() != obs_.size()) throw std::invalid_argument("Error, array contains duplicate observations.");   // DOPG:44-45
    }
    // dispersion: row-major m x m (the reference takes an UpperSPDPackMatrix, DOPG:48-61)
    DirectlyObservedParameterGroup(std::vector<double> dispersion, std::vector<ObservationParameter *> obs)
        : DirectlyObservedParameterGroup(std::move(obs)) {
        const size_t m = obs_.size();
        if (dispersion.size() != m * m) throw std::invalid_argument("Error, number of observations and number of rows/columns in dispersion matrix are unequal");
        for (size_t r = 0; r < m; r++) obs_[r]->setVariance(dispersion[r * m + r]);
        disp_ = std::move(dispersion);
    }
    bool hasFullyPopulatedWeightMatrix() const { return !disp_.empty(); }
    int getNumberOfParameters() const { return (int)obs_.size(); }
    std::vector<ObservationParameter *> &observations() { return obs_; }
    const std::vector<double> &dispersion() const { return disp_; }
private:
    std::vector<ObservationParameter *> obs_;
    std::vector<double> disp_;
};

// defect/RankDefect.java
class RankDefect {
public:
    enum class DefectType { NOT_SET, FREE, FIXED };
    void reset() { tx = ty = tz = rx = ry = rz = mxyz = DefectType::NOT_SET; }
    static DefectType norm(DefectType d) { return d == DefectType::FIXED ? DefectType::FIXED : DefectType::FREE; }
    void setScale(DefectType d) { mxyz = norm(d); }
    void setRotationX(DefectType d) { rx = norm(d); }
    void setRotationY(DefectType d) { ry = norm(d); }
    void setRotationZ(DefectType d) { rz = norm(d); }
    void setTranslationX(DefectType d) { tx = norm(d); }
    void setTranslationY(DefectType d) { ty = norm(d); }
    void setTranslationZ(DefectType d) { tz = norm(d); }
    bool estimateScale() const { return mxyz == DefectType::FREE; }
    bool estimateRotationX() const { return rx == DefectType::FREE; }
    bool estimateRotationY() const { return ry == DefectType::FREE; }
    bool estimateRotationZ() const { return rz == DefectType::FREE; }
    bool estimateTranslationX() const { return tx == DefectType::FREE; }
    bool estimateTranslationY() const { return ty == DefectType::FREE; }
    bool estimateTranslationZ() const { return tz == DefectType::FREE; }
    int getDefect() const {
        return estimateScale() + estimateRotationX() + estimateRotationY() + estimateRotationZ() + estimateTranslationX() +
               estimateTranslationY() + estimateTranslationZ();
    }
    bool allFixed() const { return getDefect() == 0; }
    int flags() const {
        return (estimateTranslationX() ? JAICOV_DATUM_TX : 0) | (estimateTranslationY() ? JAICOV_DATUM_TY : 0) |
               (estimateTranslationZ() ? JAICOV_DATUM_TZ : 0) | (estimateRotationX() ? JAICOV_DATUM_RX : 0) |
               (estimateRotationY() ? JAICOV_DATUM_RY : 0) | (estimateRotationZ() ? JAICOV_DATUM_RZ : 0) |
               (estimateScale() ? JAICOV_DATUM_SCALE : 0);
    }
private:
    DefectType rx = DefectType::NOT_SET, ry = DefectType::NOT_SET, rz = DefectType::NOT_SET, tx = DefectType::NOT_SET,
               ty = DefectType::NOT_SET, tz = DefectType::NOT_SET, mxyz = DefectType::NOT_SET;
};

class BundleAdjustment;
class AdjustmentResultWritable {                                   // util/io/writer/AdjustmentResultWritable.java:36
public:
    virtual ~AdjustmentResultWritable() = default;
    virtual void exportResults(BundleAdjustment &bundleAdjustment) = 0;      // `export` is a C++ keyword
    virtual std::string toString() const = 0;
};

// BundleAdjustment.java
class BundleAdjustment {
public:
    using Listener = std::function<void(const std::string &name, double oldValue, double newValue)>;   // PropertyChangeListener

    BundleAdjustment() = default;
    ~BundleAdjustment() { if (engine_) jaicov_neq_destroy(engine_); }
    BundleAdjustment(const BundleAdjustment &) = delete;

    void add(Camera *c) { cameras_.push_back(c); }                                      // BA:652-655
    void add(ScaleBar *s) { if (std::find(scaleBars_.begin(), scaleBars_.end(), s) == scaleBars_.end()) scaleBars_.push_back(s); }
    void add(DirectlyObservedParameterGroup *g) { if (std::find(groups_.begin(), groups_.end(), g) == groups_.end()) groups_.push_back(g); }
    void addPropertyChangeListener(Listener l) { listeners_.push_back(std::move(l)); }

    void setEstimationType(EstimationType t) { estimationType_ = t; }                   // BA:1132
    void setInvertNormalEquation(MatrixInversion m) { inversion_ = m; }                 // BA:1146
    MatrixInversion getInvertNormalEquation() const { return inversion_; }
    void useCentroidedCoordinates(bool b) { centroided_ = b; }                          // BA:1181
    void centroidCoordinates(bool invert);    // BA:115-201 (private in the reference; public here so that the parity tests can call it)
    void applyAposterioriVarianceOfUnitWeight(bool b) { applyAposteriori_ = b; }        // BA:1185
    void setLevenbergMarquardtDampingValue(double l) { damping_ = std::fabs(l); }       // BA:1189
    double getLevenbergMarquardtDampingValue() const { return damping_; }
    void setMaximalNumberOfIterations(int n) { maxIter_ = n; }
    void setDevice(int d) { device_ = d; }
    void setAdjustmentResultWriter(AdjustmentResultWritable *w) { resultWriter_ = w; }   // BA:1123 (not owned)
    void interrupt() { interrupt_ = true; }                                             // BA:1455

    int getNumberOfObservations() const { return numberOfObservations_; }
    int getNumberOfUnknownParameters() const { return numberOfUnknownParameters_; }
    int getNumberOfDatumConditions() const { return rankDefect_.getDefect(); }
    int getDegreeOfFreedom() const { return numberOfObservations_ - numberOfUnknownParameters_ + rankDefect_.getDefect(); }   // BA:1080
    double getVarianceFactorApriori() const { return sigma2apriori_; }
    double getVarianceFactorAposteriori() const {                                       // BA:1090-1093
        const int dof = getDegreeOfFreedom();
        return dof > 0 && omega_ > 0 && estimationType_ != EstimationType::SIMULATION && applyAposteriori_ ? std::fabs(omega_ / (double)dof)
                                                                                                            : sigma2apriori_;
    }
    double getOmega() const { return omega_; }
    int getIterations() const { return iterationStep_; }
    const RankDefect &getRankDefect() const { return rankDefect_; }
    std::vector<ObjectCoordinate *> &getObjectCoordinates() { return objectCoordinates_; }
    std::vector<Camera *> &getCameras() { return cameras_; }
    // packed UPLO='U' cofactor matrix, order u + d (UpperSymmPackMatrix.getData()); empty for MatrixInversion.NONE (BA:1177)
    // The host copy is made on first use: the writers and most callers need a few hundred entries, which cofactorSub
    // gathers on the device, not the 1.3 GB packed array.
    const std::vector<double> &getCofactorMatrix() const { fetchCofactor(); return Qxx_; }
    double cofactor(int r, int c) const {
        fetchCofactor();
        if (r > c) std::swap(r, c);
        return Qxx_.at((size_t)r + (size_t)c * (c + 1) / 2);
    }
    // what the writers test: cofactor != null && numRows >= u + d (MatlabResultWriter.java:72, DefaultResultWriter.java:128)
    bool hasCofactorMatrix() const { return inversion_ != MatrixInversion::NONE && (qxxOnDevice_ || !Qxx_.empty()); }
    // scale * Qxx[idx, idx], row-major k x k, gathered on the device (jaicov_neq_get_dispersion_sub)
    std::vector<double> cofactorSub(const std::vector<int32_t> &idx, double scale = 1.0) const;
    // residuals v, residual cofactors qvv, redundancy numbers r and test values t of every observation row, in row order (BA:670-771),
    // on the engine of the last estimateModel (jaicov_rel_run with a zero step: v at the adjusted values).  Needs MatrixInversion.FULL.
    // sigma2Test = getVarianceFactorAposteriori() gives Pope's tau, the a-priori factor Baarda's w-test (include/jaicov_reliability.h).
    struct ObservationReliability {
        std::vector<double> v, qvv, r, t;
    };
    ObservationReliability observationReliability(double sigma2Test) const;
    // What taking an image point out would do, for every image point in the order of the images' image coordinates (the order of
    // the rows above, one entry per pair): the columns of include/jaicov_reliability_points.h, from jaicov_rel_run_points with a zero
    // step, the Omega and the degrees of freedom of the finished estimateModel.  lambda0: the non-centrality behind the minimal
    // detectable bias and the external reliability (17.075 is Baarda's value for alpha 0.1 % and power 80 %).  Needs MatrixInversion.FULL.
    struct ImagePointReliability {
        std::vector<double> q, Tprio, Tpost, nablaX, nablaY, Mxx, Mxy, Myy, mdbMajor, mdbMinor, deltaExt, dX, dY, dZ;
    };
    ImagePointReliability imagePointReliability(double sigma2Test, double lambda0 = 17.075) const;
    // The cofactor matrix of the last estimateModel re-expressed, on the device, in the datum of the points whose isDatum() flag is
    // set NOW (Baarda's S-transformation, include/jaicov_datum.h): re-flag the points, then call.  Needs a free network (d > 0)
    // and MatrixInversion FULL or REDUCED; cofactorSub, getCofactorMatrix and the writers see the new datum afterwards.
    void transformDatum();
    // Precision figures read on the device from the cofactor matrix of the last estimateModel (include/jaicov_precision.h; after
    // transformDatum they speak of the new datum).  table: one row of `columns` entries per item, in the header's order; status: its
    // JAICOV_PREC_* bits.  An empty index list means every object point / every image.  k3, k2: the caller's expansion factors of the
    // ellipsoid and of the horizontal ellipse.  Indices are the engine's: ObjectCoordinate::index, and the images in the order of flat.eo_col.
    struct PrecisionTable {
        int columns = 0;
        std::vector<double> table;
        std::vector<int32_t> status;
    };
    PrecisionTable pointPrecision(double sigma2, double k3 = 1.0, double k2 = 1.0, const std::vector<int32_t> &points = {}) const;
    PrecisionTable stationPrecision(double sigma2, double k3 = 1.0, double k2 = 1.0, const std::vector<int32_t> &images = {}) const;   // needs MatrixInversion.FULL
    // pairs: (A, B) point indices, flattened; rows of L, sigma_L, sigma of the three coordinate differences
    PrecisionTable lengthPrecision(double sigma2, const std::vector<int32_t> &pairs) const;
    // The k <= 4 largest eigenpairs of the principal sub-block over columns [firstCol, firstCol + nCols) by subspace iteration
    struct PrincipalComponents {
        std::vector<double> values, vectors, residuals;      // vectors: k rows of nCols entries
        double trace = 0.0;
        int iterations = 0;
        bool converged = false;
    };
    PrincipalComponents principalComponents(int firstCol, int nCols, int k, double tol = 0.0, int maxIterations = 200) const;
    // Correlations and significance tests of the unknowns, read on the device from the cofactor matrix of the last estimateModel
    // (include/jaicov_parameters.h; after transformDatum they speak of the new datum).  Columns are those of the cofactor matrix,
    // slots those of the flat problem; pairMask bit 4 a + b: a column of class a considers partners of class b (JAICOV_PAR_CLASS_*).
    struct ParameterCorrelations {
        std::vector<double> rho;                 // one entry per column: the coefficient with its worst partner (NaN: none)
        std::vector<int32_t> partner, status;    // -1: none; JAICOV_PAR_NONPOSITIVE / _NOT_FINITE
    };
    ParameterCorrelations parameterCorrelations(uint32_t pairMask = 0xFFFF, uint32_t flags = 0) const;
    struct CorrelatedPairs {
        int64_t count = 0;                       // always exact; cols and rho are empty when it exceeds the capacity
        std::vector<int32_t> cols;               // i, j (i > j) of every pair, sorted by |rho| descending, then i, then j
        std::vector<double> rho;
    };
    CorrelatedPairs correlatedPairs(double threshold, uint32_t pairMask = 0xFFFF, uint32_t flags = 0, int64_t capacity = 1 << 16) const;
    // rho between every column of rowCols and every column of colCols, row-major rowCols.size() x colCols.size()
    std::vector<double> correlationBlock(const std::vector<int32_t> &rowCols, const std::vector<int32_t> &colCols) const;
    // test of x_g = x0_g: group g has the slots groupSlot[groupBegin[g] .. groupBegin[g + 1]); x0 empty = zeros
    struct ParameterTests {
        std::vector<double> table;               // rows of q, T = q / (k sigma2), k, t (JAICOV_PAR_TEST_COLUMNS)
        std::vector<int32_t> status;             // JAICOV_PAR_* bits of every group
    };
    ParameterTests testParameters(double sigma2, const std::vector<int32_t> &groupBegin, const std::vector<int32_t> &groupSlot,
                                  const std::vector<double> &x0 = {}) const;
    // Planes, spheres, lines and circles through adjusted object points, fitted on the device with the members' whole block of the
    // cofactor matrix (include/jaicov_forms.h).  Form g has the type formType[g] (JAICOV_FORM_*) and the points
    // formPoint[formBegin[g] .. formBegin[g + 1]) (ObjectCoordinate::index).
    struct FormFits {
        std::vector<double> table;               // rows of JAICOV_FORM_COLUMNS: parameters, sigma, Omega, f, T, distances, iterations
        std::vector<double> qpp;                 // rows of JAICOV_FORM_QPP_COLUMNS: Q_pp, packed upper 7 x 7
        std::vector<double> members;             // rows of JAICOV_FORM_MEMBER_COLUMNS parallel to formPoint: v, distance, nabla, T_i
        std::vector<int32_t> status, memberStatus;
    };
    FormFits fitForms(double sigma2, const std::vector<int32_t> &formType, const std::vector<int32_t> &formBegin,
                      const std::vector<int32_t> &formPoint, int maxIterations = 20, double tol = 0.0) const;
    // The same with cylinders and cones (JAICOV_SURF_*) and with start values (include/jaicov_surfaces.h): start is empty or holds
    // seven values per form, the reported parameters in the engine's frame; a row that begins with NaN lets the form find its own.
    FormFits fitSurfaces(double sigma2, const std::vector<int32_t> &formType, const std::vector<int32_t> &formBegin,
                         const std::vector<int32_t> &formPoint, const std::vector<double> &start = {}, int maxIterations = 20,
                         double tol = 0.0) const;
    // Image space (include/jaicov_predict.h), read on the device from the cofactor matrix of the last estimateModel; needs
    // MatrixInversion.FULL.  A pair is (image, point): the images in the order of flat.eo_col, ObjectCoordinate::index.
    // predictImagePoints: where the adjusted point appears in the image, with J Qxx J', sigmas and the ellipse (rows of JAICOV_PRED_POINT_COLUMNS).
    struct ImageTable {
        int columns = 0;
        std::vector<double> table;
        std::vector<int32_t> status;             // JAICOV_PRED_* bits of every pair
    };
    ImageTable predictImagePoints(double sigma2, const std::vector<int32_t> &images, const std::vector<int32_t> &points, double k2 = 1.0) const;
    // checkImagePoints: the test of measurements xy (two per pair) that were withheld from the adjustment, with their dispersions
    // disp (var_x, var_y, rho per pair); sigma2Post <= 0: the a-priori factor.  groupBegin empty: no groups; otherwise a CSR over the pairs.
    struct ImageCheck {
        std::vector<double> table;               // rows of JAICOV_PRED_CHECK_COLUMNS: d, M, q, T_prio, T_post
        std::vector<int32_t> status;
        std::vector<double> groups;              // rows of JAICOV_PRED_GROUP_COLUMNS: q_G, T_prio, T_post, 2 m
        std::vector<int32_t> groupStatus;
    };
    ImageCheck checkImagePoints(const std::vector<int32_t> &images, const std::vector<int32_t> &points, const std::vector<double> &xy,
                                const std::vector<double> &disp, double sigma2Post = 0.0, const std::vector<int32_t> &groupBegin = {}) const;
    // Object space (include/jaicov_newpoints.h): object points that were not part of the adjustment, intersected from measurements
    // xy (two per ray) with the dispersions disp (var_x, var_y, rho per ray) in the images rayImage (the order of flat.eo_col) of the
    // adjusted block, read on the device from the cofactor matrix of the last estimateModel; needs MatrixInversion.FULL.  rayBegin is
    // the CSR of the points' rays, start holds X, Y, Z of every point.  pairs (two members per pair; >= 0: a new point of the call,
    // -1 - P: object point P of the block) asks for lengths with their correlations.
    struct NewPoints {
        std::vector<double> table;               // rows of JAICOV_NEWPT_COLUMNS: X Y Z, Q_meas, Q_XX, Omega, 2m - 3, sigmas
        std::vector<int32_t> status, iterations; // JAICOV_NEWPT_* bits and the Gauss-Newton steps of every point
        std::vector<double> rayW;                // the final misclosures, two per ray
        std::vector<double> lengths;             // rows of JAICOV_NEWPT_PAIR_COLUMNS: L, sigma_L, sigma of D, q_L, q_L without the cross block
        std::vector<int32_t> lengthStatus;       // JAICOV_NEWPT_PAIR_* bits
    };
    NewPoints intersectNewPoints(double sigma2, const std::vector<int32_t> &rayBegin, const std::vector<int32_t> &rayImage,
                                 const std::vector<double> &xy, const std::vector<double> &disp, const std::vector<double> &start,
                                 const std::vector<int32_t> &pairs = {}, int maxIterations = 20) const;
    // Variance components of groups of observations (include/jaicov_vce.h) on the engine of the last estimateModel, at the adjusted
    // values (a zero step); needs MatrixInversion.FULL.  A group is a union of weight blocks: ip names the group of every image
    // point (in the order of the rows, one entry per pair), sb of every scale bar, dg of every directly observed group; -1: in no
    // group; an empty vector: none of that kind.  The image points of an image with a joint dispersion must share one group.
    struct VarianceGroups {
        std::vector<int32_t> ip, sb, dg;
        int nGroups = 0;
    };
    struct VarianceComponents {
        std::vector<double> table;               // JAICOV_VCE_COLUMNS rows of nGroups entries: n_g, Omega_g, r_g, s2_g, k_g, sd(k_g)
        std::vector<int32_t> status;             // JAICOV_VCE_* bits of every group
        double omega = 0, sumR = 0, rowsGrouped = 0, rowsUngrouped = 0, damping = 0;   // the totals over all rows
        double k(int g) const { return table[4 * status.size() + g]; }
    };
    VarianceComponents varianceComponents(const VarianceGroups &groups, double sigma2Test = 0.0) const;   // sigma2Test <= 0: the a-priori factor
    // the groups "by kind" (image points, scale bars, directly observed rows) and "by image" of the flattened problem
    VarianceGroups varianceGroupsByKind() const;
    VarianceGroups varianceGroupsByImage() const;
    // The camera in image space (include/jaicov_calibration.h), read on the device from the cofactor matrix of the last
    // estimateModel; MatrixInversion.REDUCED serves as well as FULL.  A node is (xs, ys): ideal coordinates relative to the principal
    // point at the camera's current c (two per node in xy); cameras in the order of flat.io_col.  depth empty: N = -c.
    // calibrationField: the image correction at every node with J Q J' over the camera's selected columns, sigmas, the ellipse and
    // the radial and tangential components (rows of JAICOV_CALIB_FIELD_COLUMNS); withJacobian: the camera part of every row as well.
    struct CalibrationField {
        std::vector<double> table;               // rows of JAICOV_CALIB_FIELD_COLUMNS
        std::vector<double> jacobian;            // 2 x JAICOV_CALIB_MAX_COLUMNS per node, or empty
        std::vector<int32_t> status;             // JAICOV_CALIB_* bits of every node
    };
    CalibrationField calibrationField(double sigma2, const std::vector<int32_t> &cameras, const std::vector<double> &xy,
                                      const std::vector<double> &depth = {}, double k2 = 1.0, uint32_t columns = JAICOV_CALIB_ALL,
                                      bool withJacobian = false) const;
    // compareCalibration: the difference field of camera camA and either camera camB of the same adjustment (refValues empty) or the
    // values refValues (x0, y0, c, then the coefficients of camB's table) with the covariance refCov (empty: none); sigma2Post <= 0:
    // the a-priori factor.  The summary is formed on the device.
    struct CalibrationCompare {
        std::vector<double> table;               // rows of JAICOV_CALIB_COMPARE_COLUMNS: d, C_d, q, T_prio, T_post
        std::vector<int32_t> status;
        double summary[JAICOV_CALIB_SUMMARY_COLUMNS] = {0, 0, 0, 0, 0, 0, 0, 0};
    };
    CalibrationCompare compareCalibration(int camA, int camB, const std::vector<double> &xy, const std::vector<double> &depth = {},
                                          const std::vector<double> &refValues = {}, const std::vector<double> &refCov = {},
                                          double sigma2Post = 0.0, bool relative = false) const;
    // x0, y0, c and the coefficients of camera `cam` at the engine's current values: a reference set for compareCalibration
    std::vector<double> cameraValues(int cam) const;
    const std::string &lastError() const { return lastError_; }
    jaicov_engine *nativeEngine() const { return engine_; }     // the engine of the last estimateModel (null before)

    // ---- index contract -----------------------------------------------------------------------------------
    void prepareUnknownParameters();          // BA:667-782
    void flatten();                           // object graph -> jaicov_problem_desc arrays
    EstimationStateType estimateModel();      // BA:203-387

    // flattened arrays (kept public for the parity tests)
    struct Flat {
        std::vector<int32_t> point_col, io_col, cam_dist_begin, dist_kind, dist_order, dist_col, image_camera, eo_col, ip_image,
            ip_point, blk_ip_begin, sb_a, sb_b, dg_row_begin, dg_slot;
        std::vector<uint8_t> point_datum;
        std::vector<double> cam_r0, ip_x, ip_y, ip_var_x, ip_var_y, ip_rho, blk_disp, sb_len, sb_var, dg_obs, dg_var, dg_disp, values;
        std::vector<int64_t> blk_disp_offset, dg_disp_offset;
        std::vector<UnknownParameter *> slot_param;
    } flat;

private:
    void fire(const std::string &n, double a, double b) { for (auto &l : listeners_) l(n, a, b); }
    void addUnknownParameter(UnknownParameter *p) {                                    // BA:645-650
        if (p->getColumn() == COLUMN_NOT_SET && !unknownSet_.count(p)) {
            p->setColumn(numberOfUnknownParameters_++);
            unknownSet_.insert(p);
            unknownParameters_.push_back(p);
        }
    }
    void addObjectCoordinate(ObjectCoordinate *oc) {
        if (ocSet_.insert(oc).second) objectCoordinates_.push_back(oc);
    }
    void noteVariance(double v) { sigma2apriori_ = std::min(sigma2apriori_, v); }      // BA:641
    void detectRankDefect();                  // BA:836-1042
    void pushValues();                        // objects -> flat.values
    void pullValues(const std::vector<double> &v);

    std::vector<Camera *> cameras_;
    std::vector<ScaleBar *> scaleBars_;
    std::vector<DirectlyObservedParameterGroup *> groups_;
    std::vector<ObjectCoordinate *> objectCoordinates_;
    std::unordered_set<ObjectCoordinate *> ocSet_;
    std::vector<UnknownParameter *> unknownParameters_;
    std::unordered_set<UnknownParameter *> unknownSet_;
    std::vector<Listener> listeners_;
    RankDefect rankDefect_;
    EstimationType estimationType_ = EstimationType::L2NORM;
    MatrixInversion inversion_ = MatrixInversion::FULL;
    int maxIter_ = 5000, iterationStep_ = 0, numberOfUnknownParameters_ = 0, numberOfObservations_ = 0, device_ = 0;
    bool interrupt_ = false, applyAposteriori_ = true, centroided_ = true, prepared_ = false;
    double damping_ = 0.0, omega_ = 0.0, sigma2apriori_ = 1.0, maxAbsDx_ = 0.0;
    double centroid_[3] = {0, 0, 0};
    mutable std::vector<double> Qxx_;
    mutable bool qxxOnDevice_ = false;    // an inverse is on the device and Qxx_ has not been fetched yet
    void fetchCofactor() const;
    AdjustmentResultWritable *resultWriter_ = nullptr;
    std::string lastError_;
    jaicov_engine *engine_ = nullptr;
};

// adjustment/bundle/tranformation/CoordinateTransformationExteriorOrientation.java (CTEO) on the device (include/jaicov_transform.h).
// transform() takes the BundleAdjustment whose engine holds Qxx in place of the reference's CoVar; it needs MatrixInversion.FULL.
// imagesToAlign is the reference's Map<Image, ArrayList<Image>> in iteration order.  The coordinates are in the frame of the objects'
// values (the engine's values plus the centroid shift when estimateModel centred them, BA:115-201: a translation moves X_T by the
// same shift); the covariance is sigma2 J Qxx J' packed 'U', copied to the host once per transform (a host that needs only blocks
// uses jaicov_xform_get_covariance_sub on nativeEngine()).  A fixed parameter contributes no column (the reference throws).
class CoordinateTransformationExteriorOrientation {
public:
    static CoordinateTransformationExteriorOrientation &getInstance() {                // CTEO:45-47
        static CoordinateTransformationExteriorOrientation trans;
        return trans;
    }
    CoordinateTransformationExteriorOrientation(const CoordinateTransformationExteriorOrientation &) = delete;
    CoordinateTransformationExteriorOrientation &operator=(const CoordinateTransformationExteriorOrientation &) = delete;
    void transform(const std::vector<ObjectCoordinate *> &objectCoordinatesToTransform,
                   const std::vector<std::pair<Image *, std::vector<Image *>>> &imagesToAlign, double sigma2, BundleAdjustment &adjustment);
    const std::vector<double> &getCovarianceMatrix() const { return covariance_; }     // CTEO:123-125 (UpperSymmPackMatrix.getData())
    std::vector<ObjectCoordinate *> getTransformedCoordinates() const {               // CTEO:127-129, named "<point> <image id> <reference id>"
        std::vector<ObjectCoordinate *> v;
        for (auto &c : transformed_) v.push_back(c.get());
        return v;
    }
private:
    CoordinateTransformationExteriorOrientation() = default;
    std::vector<std::unique_ptr<ObjectCoordinate>> transformed_;
    std::vector<double> covariance_;
};

// dlt/DLTCoefficients.java: the 20 parameters of one image's DLT in the reference's iteration order (b11..b33, x0, y0, c,
// X0, Y0, Z0, omega, phi, kappa).  status / solves: the device's outcome of the last adjust (include/jaicov_dlt.h, not in the reference).
class DLTCoefficients {
public:
    DLTCoefficients(const DLTCoefficients &) = delete;
    DLTCoefficients &operator=(const DLTCoefficients &) = delete;
    explicit DLTCoefficients(Image *image);
    UnknownParameter &get(ParameterType t);
    UnknownParameter *at(int i) { return p_[i].get(); }
    Image *getReference() const { return image_; }
    int status = -1;
    int solves = 0;
private:
    Image *image_;
    std::vector<std::unique_ptr<UnknownParameter>> p_;
};

// dlt/DirectLinearTransformation.java (DT) on the device (include/jaicov_dlt.h).  adjust() keeps the reference's signature and bool
// result; adjustAll() makes one device call for every image.  Homologous points are selected by name, in each image's order (DT:73-94);
// the map's X, Y, Z are used.  A device error (no GPU, out of memory) throws std::runtime_error.  The values follow the ABI: Q2 (a fixed
// x0 / y0 / c comes back as the camera's value) and Q3 (NaN after a failure), see DESIGN.md 6b.
class DirectLinearTransformation {
public:
    enum class RestrictionType {                 // DT:51-58
        IDENTICAL_PRINCIPLE_DISTANCE, ROTATION_WITHOUT_SHEAR, FIXED_PRINCIPLE_DISTANCE_X, FIXED_PRINCIPLE_DISTANCE_Y,
        FIXED_PRINCIPAL_POINT_X, FIXED_PRINCIPAL_POINT_Y
    };
    static bool adjust(DLTCoefficients &coefficients, const std::map<std::string, ObjectCoordinate *> &objectCoordinates,
                       const std::vector<RestrictionType> &restrictions = {});
    static std::vector<bool> adjustAll(const std::vector<DLTCoefficients *> &coefficients,
                                       const std::map<std::string, ObjectCoordinate *> &objectCoordinates,
                                       const std::vector<RestrictionType> &restrictions = {});
    // Start values: X0 .. kappa of an adjusted image into an ExteriorOrientation.  Q1: the DLT's c is always positive, so for a camera
    // with c < 0 (AICON) kappa + pi (wrapped into (-pi, pi]) is written.  Interior orientation is not touched.
    static void applyExteriorOrientation(DLTCoefficients &coefficients, ExteriorOrientation &eo);
    static int getMaximalNumberOfIterations() { return maximalNumberOfIterations_; }
    static void setMaximalNumberOfIterations(int n) { maximalNumberOfIterations_ = n; }
private:
    static inline int maximalNumberOfIterations_ = 5000;     // DefaultValue.getMaximalNumberOfIterations()
};

// Spatial forward intersection of object points from oriented images on the device (include/jaicov_intersect.h).  The reference has no
// counterpart: it reads the start values of its object points from a file.  intersectAll() makes one device call for every
// ObjectCoordinate that an image of `cameras` observes.  The points come in first-seen order (cameras, their images, each image's
// coordinates: the order in which BA:667-782 numbers them); a point's rays are its image coordinates in that same order, with their
// variances and correlation coefficient; interior and exterior orientation are the cameras' and images' current values (no distortion).
// X, Y, Z are written into every point whose status is JAICOV_ISECT_OK or JAICOV_ISECT_NOT_CONVERGED; the other points keep their values.
// A device error (no GPU, out of memory) throws std::runtime_error.
class ForwardIntersection {
public:
    struct Result {
        ObjectCoordinate *point = nullptr;
        int status = -1, iterations = 0, rays = 0, raysUsed = 0;
        double values[JAICOV_ISECT_OUT_PER_POINT] = {};      // X, Y, Z, qXX, qXY, qXZ, qYY, qYZ, qZZ, Omega, largest angle
    };
    static std::vector<Result> intersectAll(const std::vector<Camera *> &cameras, double sigma2apriori = 1.0, double rejectThreshold = 0.0,
                                            int minRays = 3);
    static int getMaximalNumberOfIterations() { return maximalNumberOfIterations_; }
    static void setMaximalNumberOfIterations(int n) { maximalNumberOfIterations_ = n; }
private:
    static inline int maximalNumberOfIterations_ = 50;
};

// Spatial resection of images from known object points on the device (include/jaicov_resect.h).  The reference has no counterpart.
// resectAll() makes one device call for every image of `cameras`, in the cameras' and their images' order.  An image's observations
// are its image coordinates in its own order, with their variances and correlation coefficient; the object points are the current
// values of the coordinates' ObjectCoordinates, taken as free of error; the interior orientation is the camera's (no distortion).
// With fromCurrentValues the images' current exterior orientations are the start values, otherwise every image takes the linear
// start.  X0 .. kappa are written into every image whose status is JAICOV_RESECT_OK or JAICOV_RESECT_NOT_CONVERGED; the other images
// keep their values.  A device error (no GPU, out of memory) throws std::runtime_error.
class SpatialResection {
public:
    struct Result {
        Image *image = nullptr;
        int status = -1, iterations = 0, startKind = 0, points = 0, pointsUsed = 0;
        double values[JAICOV_RESECT_OUT_PER_IMAGE] = {};     // X0, Y0, Z0, omega, phi, kappa, the upper triangle of Q, Omega
    };
    static std::vector<Result> resectAll(const std::vector<Camera *> &cameras, bool fromCurrentValues = false, double sigma2apriori = 1.0,
                                         double rejectThreshold = 0.0, int minPoints = 4);
    static int getMaximalNumberOfIterations() { return maximalNumberOfIterations_; }
    static void setMaximalNumberOfIterations(int n) { maximalNumberOfIterations_ = n; }
private:
    static inline int maximalNumberOfIterations_ = 50;
};

// Relative orientation of image pairs from their common image points on the device (include/jaicov_relorient.h).  The reference has
// no counterpart.  orientAll() makes one device call for every pair (a, b).  A pair's observations are the image coordinates of the
// ObjectCoordinates both images observe, in the order of image a's coordinates, with their variances and correlation coefficients;
// the interior orientations are those of the images' cameras (no distortion).  With fromCurrentValues the current exterior
// orientation of image b relative to that of image a is the start value, otherwise every pair takes the linear starts.  Nothing is
// written into the images: apply() puts image a at the origin with zero angles and image b at the result, its X0 times baseLength,
// where the status is JAICOV_RELOR_OK or JAICOV_RELOR_NOT_CONVERGED.  A device error (no GPU, out of memory) throws std::runtime_error.
class RelativeOrientation {
public:
    struct Result {
        Image *a = nullptr, *b = nullptr;
        int status = -1, iterations = 0, startKind = 0, points = 0, pointsUsed = 0;
        double values[JAICOV_RELOR_OUT_PER_PAIR] = {};       // X0, Y0, Z0 (unit length), omega, phi, kappa, the upper triangle of Q, Omega
    };
    static std::vector<Result> orientAll(const std::vector<std::pair<Image *, Image *>> &pairs, bool fromCurrentValues = false,
                                         double sigma2apriori = 1.0, double rejectThreshold = 0.0, int minPoints = 6);
    static bool apply(const Result &result, double baseLength = 1.0);
    static int getMaximalNumberOfIterations() { return maximalNumberOfIterations_; }
    static void setMaximalNumberOfIterations(int n) { maximalNumberOfIterations_ = n; }
private:
    static inline int maximalNumberOfIterations_ = 50;
};

// Absolute orientation on the device (include/jaicov_simil.h): the spatial similarity transformation that carries a model onto a
// target frame.  The reference has no counterpart.  estimateAll() makes one device call for every model.  A model's source
// coordinates are the current values of its ObjectCoordinates, `target` holds the same points in the target frame (control points, or
// another model); cofSource and cofTarget hold qXX qXY qXZ qYY qYZ qZZ per point, as ForwardIntersection returns them, and an empty
// one means error-free (source) or the unit matrix (target).  Nothing is written into the points: apply() carries the given points
// and the exterior orientations of the given images into the target frame with a result whose status is JAICOV_SIMIL_OK or
// JAICOV_SIMIL_NOT_CONVERGED; the dispersion of the seven parameters is not propagated.  A device error (no GPU, out of memory) throws
// std::runtime_error.
class SimilarityTransformation {
public:
    struct Model {
        std::vector<ObjectCoordinate *> points;
        std::vector<std::array<double, 3>> target;
        std::vector<std::array<double, 6>> cofSource, cofTarget;
    };
    struct Result {
        int status = -1, iterations = 0, startKind = 0, points = 0, pointsUsed = 0;
        double values[JAICOV_SIMIL_OUT_PER_MODEL] = {};      // Tx, Ty, Tz, m, omega, phi, kappa, the upper triangle of Q, Omega
        std::vector<bool> used;                              // per point of the model
        std::vector<double> q;
    };
    static std::vector<Result> estimateAll(const std::vector<Model> &models, double rejectThreshold = 0.0, int minPoints = 3);
    static bool apply(const Result &result, const std::vector<ObjectCoordinate *> &points, const std::vector<Image *> &images);
    static int getMaximalNumberOfIterations() { return maximalNumberOfIterations_; }
    static void setMaximalNumberOfIterations(int n) { maximalNumberOfIterations_ = n; }
private:
    static inline int maximalNumberOfIterations_ = 50;
};

// Lens-distortion correction on the device (include/jaicov_lens.h): the measured image coordinates of a camera reduced to those of the
// distortion-free camera, with their 2 x 2 dispersion, and the inverse that applies the camera's distortion models to ideal
// coordinates.  The reference has no counterpart.  Each call takes every image coordinate of the camera, image by image in insertion
// order, with the current values of the interior orientation and of the distortion coefficients, and makes one device call.
// Distance-dependent coefficients (Di) are left out unless withDistance: then N of every point (PDF:151) is formed from the current
// values of its object point and of the image's exterior orientation; a point whose N is not finite (no values yet) or 0 comes back
// JAICOV_LENS_NOT_FINITE.  Nothing is written into the coordinates: Scope does that for
// as long as it lives.  A device error (no GPU, out of memory) throws std::runtime_error.
class LensCorrection {
public:
    struct Result {
        ImageCoordinate *coordinate = nullptr;
        double x = 0, y = 0, varianceX = 0, varianceY = 0, rho = 0;
        int status = -1, iterations = 0;
    };
    static std::vector<Result> correctAll(Camera &camera, bool withDistance = false, double tolerance = 0.0);
    static std::vector<Result> distortAll(Camera &camera, bool withDistance = false);
    static int getMaximalNumberOfIterations() { return maximalNumberOfIterations_; }
    static void setMaximalNumberOfIterations(int n) { maximalNumberOfIterations_ = n; }

    // writes the results whose status is JAICOV_LENS_OK or JAICOV_LENS_NOT_CONVERGED into their ImageCoordinates (values, variances,
    // rho) and puts the former ones back when it goes out of scope
    class Scope {
    public:
        explicit Scope(const std::vector<Result> &results);
        ~Scope();
        Scope(const Scope &) = delete;
        Scope &operator=(const Scope &) = delete;
        int applied() const { return (int)saved_.size(); }
    private:
        void restore();
        std::vector<Result> saved_;
    };
private:
    static std::vector<Result> run(Camera &camera, bool correct, bool withDistance, double tolerance);
    static inline int maximalNumberOfIterations_ = 20;
};

}  // namespace jaicov::host
