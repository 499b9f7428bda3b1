// TEST SCAFFOLDING ONLY (oracle/Makefile, targets _ref/libref_hash.so and
// _ref/libref_store.so).
// Stand-in for libe's <e/endian.h>: little-endian pack / unpack of fixed-width
// values by memcpy, big-endian by memcpy and a byte swap, over uint8_t or char
// buffers.  Little-endian hosts only.
#ifndef e_endian_h_
#define e_endian_h_
#include <assert.h>
#include <stdint.h>
#include <string.h>

#if !defined(__BYTE_ORDER__) || __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "oracle/ref_stub/e/endian.h: little-endian hosts only"
#endif

namespace e {

template <class B, class T>
inline B* stub_pack(const T& v, B* p) {
    static_assert(sizeof(B) == 1, "byte buffer");
    memcpy(p, &v, sizeof(T));
    return p + sizeof(T);
}

template <class B, class T>
inline const B* stub_unpack(const B* p, T* v) {
    static_assert(sizeof(B) == 1, "byte buffer");
    memcpy(v, p, sizeof(T));
    return p + sizeof(T);
}

template <class B> inline B* pack32le(uint32_t v, B* p) { return stub_pack(v, p); }
template <class B> inline B* pack64le(uint64_t v, B* p) { return stub_pack(v, p); }
template <class B> inline B* packdoublele(double v, B* p) { return stub_pack(v, p); }

template <class B, class T>
inline const B* unpack32le(const B* p, T* v) {
    static_assert(sizeof(T) == 4, "32-bit destination");
    return stub_unpack(p, v);
}

template <class B, class T>
inline const B* unpack64le(const B* p, T* v) {
    static_assert(sizeof(T) == 8, "64-bit destination");
    return stub_unpack(p, v);
}

template <class B> inline const B* unpackdoublele(const B* p, double* v) { return stub_unpack(p, v); }

// big-endian (target _ref/libref_store.so): memcpy and a byte swap
template <class B> inline B* pack8be(uint8_t v, B* p) { return stub_pack(v, p); }
template <class B> inline B* pack16be(uint16_t v, B* p) { return stub_pack(__builtin_bswap16(v), p); }
template <class B> inline B* pack32be(uint32_t v, B* p) { return stub_pack(__builtin_bswap32(v), p); }
template <class B> inline B* pack64be(uint64_t v, B* p) { return stub_pack(__builtin_bswap64(v), p); }

template <class B, class T>
inline const B* unpack8be(const B* p, T* v) {
    static_assert(sizeof(T) == 1, "8-bit destination");
    return stub_unpack(p, v);
}

template <class B, class T>
inline const B* unpack16be(const B* p, T* v) {
    static_assert(sizeof(T) == 2, "16-bit destination");
    uint16_t x;
    p = stub_unpack(p, &x);
    *v = static_cast<T>(__builtin_bswap16(x));
    return p;
}

template <class B, class T>
inline const B* unpack32be(const B* p, T* v) {
    static_assert(sizeof(T) == 4, "32-bit destination");
    uint32_t x;
    p = stub_unpack(p, &x);
    *v = static_cast<T>(__builtin_bswap32(x));
    return p;
}

template <class B, class T>
inline const B* unpack64be(const B* p, T* v) {
    static_assert(sizeof(T) == 8, "64-bit destination");
    uint64_t x;
    p = stub_unpack(p, &x);
    *v = static_cast<T>(__builtin_bswap64(x));
    return p;
}

}  // namespace e
#endif
