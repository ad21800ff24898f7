// Behaving stand-in for rmagine's StopWatch: a call returns the seconds since the previous call.
#pragma once
#include <chrono>

namespace rmagine {

class StopWatch {
public:
    double operator()()
    {
        const auto now = std::chrono::steady_clock::now();
        const double s = std::chrono::duration<double>(now - m_last).count();
        m_last = now;
        return s;
    }
private:
    std::chrono::steady_clock::time_point m_last = std::chrono::steady_clock::now();
};

}  // namespace rmagine
