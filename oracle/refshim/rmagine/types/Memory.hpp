// Behaving stand-in for rmagine's Memory / MemView (host memory only) -- TEST INFRASTRUCTURE ONLY.
#pragma once
#include <cstddef>
#include <vector>

namespace rmagine {

struct RAM {};

template <typename T>
class MemView {
public:
    MemView() = default;
    MemView(T* p, size_t n) : m_ptr(p), m_n(n) {}
    T& operator[](size_t i) { return m_ptr[i]; }
    const T& operator[](size_t i) const { return m_ptr[i]; }
    T& at(size_t i) { return m_ptr[i]; }
    const T& at(size_t i) const { return m_ptr[i]; }
    T* raw() { return m_ptr; }
    const T* raw() const { return m_ptr; }
    size_t size() const { return m_n; }
protected:
    T* m_ptr = nullptr;
    size_t m_n = 0;
};

template <typename T, typename AllocT = RAM>
class Memory : public MemView<T> {
public:
    Memory() = default;
    explicit Memory(size_t n) { resize(n); }
    Memory(const Memory& o) : MemView<T>(), m_store(o.m_store) { rebind(); }
    Memory(Memory&& o) noexcept : MemView<T>(), m_store(std::move(o.m_store)) { rebind(); o.rebind(); }
    Memory& operator=(const Memory& o) { m_store = o.m_store; rebind(); return *this; }
    Memory& operator=(Memory&& o) noexcept { m_store = std::move(o.m_store); rebind(); o.rebind(); return *this; }
    void resize(size_t n) { m_store.resize(n); rebind(); }
private:
    void rebind() { this->m_ptr = m_store.data(); this->m_n = m_store.size(); }
    std::vector<T> m_store;
};

}  // namespace rmagine
