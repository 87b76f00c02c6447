// tests/native/ref_hit_records.cpp — TEST INFRASTRUCTURE ONLY (never linked into the product, run by
// no test, build() or GPU job).
//
// Records the reference's own SearchBVH HitRecord (G/include/query.h:224-311, with
// intersectTriangle's tail :110-130) for a list of rays against caller-supplied scene arrays, for
// the fixtures under tests/golden/hit_records/ (tests/golden/hit_records/meta.json has the
// commands).  It includes the reference's headers at compile time only, as oracle/ref/ref_g.cpp
// does, and is compiled by hand with the flags of oracle/Makefile's ref_g rule into the
// git-ignored oracle/_ref/:
//
//   g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -w -D__device__= \
//       -I$G/include -I$G/src -I$G/third_party/glm tests/native/ref_hit_records.cpp \
//       -x c++ $G/include/bvh.cu $G/include/query.cu -o oracle/_ref/ref_hit_records
//
//   ref_hit_records <indir> <outdir>
//     <indir>/{nodes,aabbs,tris}.bin in the reference layouts, <indir>/rays.f32 (n x 6 floats:
//     origin, direction); writes <outdir>/{hit.u8, tri.i32, t.f32, p.f32, normal.f32, front.u8}.
// Nothing here changes reference arithmetic; it only chooses inputs and writes outputs.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "query.h"

namespace {

template <class T>
bool read_bin(const std::string& path, std::vector<T>& out) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(size_t(n) / sizeof(T));
    const size_t r = out.empty() ? 0 : std::fread(out.data(), sizeof(T), out.size(), f);
    std::fclose(f);
    return r == out.size() && size_t(n) % sizeof(T) == 0;
}

template <class T>
bool write_bin(const std::string& path, const std::vector<T>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t w = v.empty() ? 0 : std::fwrite(v.data(), sizeof(T), v.size(), f);
    std::fclose(f);
    return w == v.size();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: ref_hit_records <indir> <outdir>\n");
        return 2;
    }
    const std::string indir = argv[1], outdir = argv[2];
    std::vector<BVHNode> nodes;
    std::vector<AABB> aabbs;
    std::vector<Triangle> tris;
    std::vector<float> rays;
    if (!read_bin(indir + "/nodes.bin", nodes) || !read_bin(indir + "/aabbs.bin", aabbs) ||
        !read_bin(indir + "/tris.bin", tris) || !read_bin(indir + "/rays.f32", rays) || rays.size() % 6 != 0) {
        std::fprintf(stderr, "cannot read the arrays in %s\n", indir.c_str());
        return 1;
    }
    const size_t n = rays.size() / 6;
    std::vector<uint8_t> hit(n), front(n);
    std::vector<int32_t> tri(n);
    std::vector<float> t(n), p(3 * n), normal(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const float* r = &rays[6 * i];
        const Ray ray(make_vec3(r[0], r[1], r[2]), make_vec3(r[3], r[4], r[5]));
        HitRecord rec;
        SearchBVH((int)tris.size(), ray, nodes.data(), aabbs.data(), tris.data(), rec);
        hit[i] = rec.hit ? 1 : 0;
        tri[i] = rec.triangleIdx;
        t[i] = (float)rec.t;
        p[3 * i] = rec.p.x, p[3 * i + 1] = rec.p.y, p[3 * i + 2] = rec.p.z;
        normal[3 * i] = rec.normal.x, normal[3 * i + 1] = rec.normal.y, normal[3 * i + 2] = rec.normal.z;
        front[i] = rec.front_face ? 1 : 0;
    }
    const bool ok = write_bin(outdir + "/hit.u8", hit) && write_bin(outdir + "/tri.i32", tri) && write_bin(outdir + "/t.f32", t) &&
                    write_bin(outdir + "/p.f32", p) && write_bin(outdir + "/normal.f32", normal) &&
                    write_bin(outdir + "/front.u8", front);
    return ok ? 0 : 1;
}
