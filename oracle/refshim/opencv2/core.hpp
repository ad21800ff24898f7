// Behaving stand-in for the part of OpenCV's core the reference's radar loop calls -- TEST INFRASTRUCTURE ONLY.
// Written from DESIGN.md §2 item 4 and OpenCV's public interface: `m *= s` is convertTo(m, -1, s), which multiplies each
// f32 element by the f32 value of the scalar (and adds an f32 zero); convertTo(CV_8UC1) is saturate_cast<uchar>(cvRound(x)),
// cvRound being the SSE conversion (round-half-even, NaN / out-of-range -> INT_MIN -> 0 after saturation).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <emmintrin.h>

typedef unsigned char uchar;

#define CV_8U 0
#define CV_32F 5
#define CV_64F 6
#define CV_8UC1 CV_8U
#define CV_32FC1 CV_32F
#define CV_64FC1 CV_64F

namespace cv {

struct Scalar {
    double val[4];
    Scalar(double v0 = 0, double v1 = 0, double v2 = 0, double v3 = 0) : val{v0, v1, v2, v3} {}
};

struct Size {
    int width = 0, height = 0;
    Size() = default;
    Size(int w, int h) : width(w), height(h) {}
};

inline int cvRound(float v) { return _mm_cvtss_si32(_mm_set_ss(v)); }
inline int cvRound(double v) { return _mm_cvtsd_si32(_mm_set_sd(v)); }

template <typename T> inline T saturate_cast(int v);
template <typename T> inline T saturate_cast(float v);
template <typename T> inline T saturate_cast(double v);
template <> inline uchar saturate_cast<uchar>(int v) { return (uchar)((unsigned)v <= 255u ? v : v > 0 ? 255 : 0); }
template <> inline uchar saturate_cast<uchar>(float v) { return saturate_cast<uchar>(cvRound(v)); }
template <> inline uchar saturate_cast<uchar>(double v) { return saturate_cast<uchar>(cvRound(v)); }
template <> inline float saturate_cast<float>(float v) { return v; }
template <> inline float saturate_cast<float>(double v) { return (float)v; }
template <> inline double saturate_cast<double>(float v) { return (double)v; }
template <> inline double saturate_cast<double>(double v) { return v; }

template <typename T> struct DataType;
template <> struct DataType<uchar> { enum { type = CV_8U }; };
template <> struct DataType<float> { enum { type = CV_32F }; };
template <> struct DataType<double> { enum { type = CV_64F }; };

inline size_t elem_size_of(int type) { return type == CV_8U ? 1 : type == CV_32F ? 4 : 8; }

// 2-D, one channel; a header over shared storage, so that col() is a view like OpenCV's
class Mat {
public:
    int rows = 0, cols = 0;
    uchar* data = nullptr;
    size_t step = 0;    // bytes between rows

    Mat() = default;
    Mat(int r, int c, int type) { create(r, c, type); }

    int type() const { return m_type; }
    size_t elemSize() const { return elem_size_of(m_type); }
    bool isContinuous() const { return step == (size_t)cols * elemSize() || rows <= 1; }
    bool empty() const { return rows == 0 || cols == 0 || !data; }

    void create(int r, int c, int type)
    {
        if (data && r == rows && c == cols && type == m_type) return;
        m_type = type; rows = r; cols = c;
        step = (size_t)c * elemSize();
        m_store.reset(new uchar[(size_t)r * step + 1], std::default_delete<uchar[]>());
        data = m_store.get();
    }

    // Mat::resize(sz): the number of ROWS becomes sz, the kept rows keep their content, new rows are not initialised
    void resize(size_t sz)
    {
        if ((size_t)rows == sz && data) return;
        const size_t st = (size_t)cols * elemSize();
        std::shared_ptr<uchar> fresh(new uchar[sz * st + 1], std::default_delete<uchar[]>());
        const size_t keep = sz < (size_t)rows ? sz : (size_t)rows;
        for (size_t r = 0; r < keep && data; r++) memcpy(fresh.get() + r * st, data + r * step, st);
        m_store = fresh; data = m_store.get(); step = st; rows = (int)sz;
    }

    template <typename T> T& at(int r, int c) { return *reinterpret_cast<T*>(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    template <typename T> const T& at(int r, int c) const { return *reinterpret_cast<const T*>(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    // one index: element i of a continuous matrix or of a single row, else row i of a single column
    template <typename T> T& at(int i)
    {
        if (isContinuous() || rows == 1) return reinterpret_cast<T*>(data)[i];
        return at<T>(i, 0);
    }
    template <typename T> const T& at(int i) const { return const_cast<Mat*>(this)->at<T>(i); }

    Mat col(int x) const
    {
        Mat m;
        m.rows = rows; m.cols = 1; m.m_type = m_type; m.step = step; m.m_store = m_store;
        m.data = data + (size_t)x * elemSize();
        return m;
    }

    Mat& setTo(const Scalar& s)
    {
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++) store(r, c, s.val[0]);
        return *this;
    }

    // dst(x) = saturate_cast<rtype>(src(x) * alpha + beta); rtype < 0 keeps the type.  f32 sources are scaled in f32
    // (alpha and beta narrowed first), and not at all when alpha = 1, beta = 0.  The destination is written in place
    // when it already has the right shape and type (a col() view of an image), as OpenCV does.
    void convertTo(const Mat& dst_, int rtype, double alpha = 1, double beta = 0) const
    {
        Mat& dst = const_cast<Mat&>(dst_);
        if (rtype < 0) rtype = m_type;
        if (!(dst.data && dst.rows == rows && dst.cols == cols && dst.m_type == rtype)) dst.create(rows, cols, rtype);
        const bool scaled = !(alpha == 1.0 && beta == 0.0);
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++) {
                if (m_type == CV_32F) {
                    float v = at<float>(r, c);
                    if (scaled) v = v * (float)alpha + (float)beta;
                    dst.store(r, c, v);
                } else {
                    double v = m_type == CV_8U ? (double)at<uchar>(r, c) : at<double>(r, c);
                    if (scaled) v = v * alpha + beta;
                    dst.store(r, c, v);
                }
            }
    }

protected:
    template <typename V> void store(int r, int c, V v)
    {
        if (m_type == CV_8U) at<uchar>(r, c) = saturate_cast<uchar>(v);
        else if (m_type == CV_32F) at<float>(r, c) = saturate_cast<float>(v);
        else at<double>(r, c) = saturate_cast<double>(v);
    }
    int m_type = CV_8U;
    std::shared_ptr<uchar> m_store;
};

inline Mat& operator*=(Mat& a, double s) { a.convertTo(a, -1, s); return a; }

template <typename T>
class Mat_ : public Mat {
public:
    Mat_() { m_type = DataType<T>::type; }
    Mat_(int r, int c) : Mat(r, c, DataType<T>::type) {}
    Mat_(int r, int c, const T& value) : Mat(r, c, DataType<T>::type)
    {
        for (int i = 0; i < r; i++)
            for (int j = 0; j < c; j++) Mat::at<T>(i, j) = value;
    }
    explicit Mat_(Size sz) : Mat(sz.height, sz.width, DataType<T>::type) {}
    template <typename U> U& at(int r, int c) { return Mat::at<U>(r, c); }
    template <typename U> U& at(int i) { return Mat::at<U>(i); }
    T& operator()(int r, int c) { return Mat::at<T>(r, c); }
};

template <typename T> inline Mat_<T>& operator*=(Mat_<T>& a, double s) { a.convertTo(a, -1, s); return a; }

}  // namespace cv
