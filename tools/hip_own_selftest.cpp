// Stand-alone exercise of gecco_amd/csrc/crf_hip_own.hpp on a machine WITHOUT a device, for a host sanitizer:
//
//   hipcc -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         tools/hip_own_selftest.cpp -o hip_own_selftest && ./hip_own_selftest
//
// Every HIP call fails here, so what runs is the failure path of each owner: nothing may leak, be freed twice or be left
// half-set.  With a device present it refuses to run (the success paths belong to the GPU suite).
#include <cstdio>
#include <string>
#include <utility>

#include "../gecco_amd/csrc/crf_hip_own.hpp"

namespace gecco {
static std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }
const char *last_error() { return g_error.c_str(); }
int check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return GECCO_CRF_OK;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? GECCO_CRF_ENODEV : GECCO_CRF_EHIP;
}
}  // namespace gecco

using namespace gecco;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("line %d: expected %s\n", __LINE__, #cond);         \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

struct Owner {  // the shape of the trainers and the plan: scope first, then a stream, then blocks
    DeviceScope home{DeviceScope::kLater};
    int device = -1;
    Stream stream;
    DeviceBlock<double> a, b;
    ~Owner() { home.enter(device); }
};

int main() {
    int n = 0;
    if (hipGetDeviceCount(&n) == hipSuccess && n > 0) {
        std::printf("a device is present: this program covers the no-device paths only\n");
        return 2;
    }
    EXPECT(check_device(0) == GECCO_CRF_ENODEV);
    EXPECT(std::string(last_error()) == "no HIP device available (this library has no CPU fallback)");
    EXPECT(set_device(0) != GECCO_CRF_OK && use_device(0) != GECCO_CRF_OK);
    {
        DeviceBlock<double> blk;
        EXPECT(blk.alloc(4, "alloc") != GECCO_CRF_OK && blk.get() == nullptr && blk.capacity() == 0);
        EXPECT(blk.alloc(0, "alloc") != GECCO_CRF_OK && blk.get() == nullptr);  // a second alloc on an empty block
        const std::vector<double> h = {1.0, 2.0};
        EXPECT(blk.upload(h, "upload") != GECCO_CRF_OK && blk.get() == nullptr);
        EXPECT(blk.upload(h.data(), h.size(), "upload", nullptr) != GECCO_CRF_OK && blk.get() == nullptr);
        DeviceBlock<double> moved(std::move(blk));  // move construction
        EXPECT(moved.get() == nullptr && blk.get() == nullptr);
        DeviceBlock<double> assigned;
        assigned = std::move(moved);  // move assignment
        assigned = std::move(assigned);  // ... onto itself
        EXPECT(assigned.get() == nullptr);
        EXPECT(assigned.reserve(1000, "reserve") != GECCO_CRF_OK && assigned.get() == nullptr && assigned.capacity() == 0);
        EXPECT(assigned.at<char>(0) == nullptr);
        assigned.release();
        assigned.release();  // release twice
        std::vector<DeviceBlock<char>> many(3);  // (the overlap join keeps its blocks in a vector)
        many.emplace_back();
        EXPECT(many.back().alloc(16, "alloc") != GECCO_CRF_OK);
        many.resize(40);
    }
    {
        Stream s;
        EXPECT(s.create() != GECCO_CRF_OK && s.get() == nullptr);
        EXPECT(s.create() != GECCO_CRF_OK && s.get() == nullptr);
    }
    {
        DeviceScope saved;       // save only: the save fails, so nothing is restored
        DeviceScope entered(0);  // enter: save and set both fail
        DeviceScope later(DeviceScope::kLater);
        later.enter(-1);  // no HIP call
        later.enter(0);
    }
    {
        Owner never;  // refused before the device was checked: device < 0
        Owner reached;
        reached.device = 0;
        EXPECT(reached.stream.create() != GECCO_CRF_OK);
        EXPECT(reached.a.alloc(8, "alloc") != GECCO_CRF_OK);
        EXPECT(reached.b.reserve(8, "reserve") != GECCO_CRF_OK);
    }
    std::printf(failures ? "%d expectations failed\n" : "hip_own_selftest: all expectations held\n", failures);
    return failures ? 1 : 0;
}
