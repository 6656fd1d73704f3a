// stand-in for Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h (which brings sim3.h and Eigen): the part of g2o::Sim3 that
// adapter/sim3opt/OptimizeSim3.cc touches -- the (Quaterniond, Vector3d, double) constructor, rotation(), translation(), scale() -- over
// stand-ins for the two Eigen types with Eigen's own conventions (Quaterniond(w, x, y, z); x() y() z() w(); Vector3d(x, y, z), operator[]).
// Plain data: no arithmetic, the adaptor does none on the host.
#ifndef CVSTUB_TYPES_SEVEN_DOF_EXPMAP_H
#define CVSTUB_TYPES_SEVEN_DOF_EXPMAP_H
namespace Eigen {
class Quaterniond
{
public:
    Quaterniond() : x_(0), y_(0), z_(0), w_(1) {}
    Quaterniond(double w, double x, double y, double z) : x_(x), y_(y), z_(z), w_(w) {}
    double x() const { return x_; }
    double y() const { return y_; }
    double z() const { return z_; }
    double w() const { return w_; }
private:
    double x_, y_, z_, w_;
};
class Vector3d
{
public:
    Vector3d() { v_[0] = v_[1] = v_[2] = 0; }
    Vector3d(double x, double y, double z) { v_[0] = x; v_[1] = y; v_[2] = z; }
    double operator[](int i) const { return v_[i]; }
    double &operator[](int i) { return v_[i]; }
private:
    double v_[3];
};
}
namespace g2o {
using namespace Eigen;
struct Sim3
{
    Sim3() : s(1.) {}
    Sim3(const Quaterniond &r, const Vector3d &t, double s) : r(r), t(t), s(s) {}
    inline const Vector3d &translation() const { return t; }
    inline const Quaterniond &rotation() const { return r; }
    inline const double &scale() const { return s; }
protected:
    Quaterniond r;
    Vector3d t;
    double s;
};
}
#endif
