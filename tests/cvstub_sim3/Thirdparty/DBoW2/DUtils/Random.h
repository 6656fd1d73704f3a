// stand-in for the reference's Thirdparty/DBoW2/DUtils/Random.h: the two members adapter/sim3/Sim3Solver.cc and its test driver call
// (same names and types) over a seeded 64-bit linear congruential generator, so that a test can repeat a solver's stream
#ifndef CVSTUB_DUTILS_RANDOM_H
#define CVSTUB_DUTILS_RANDOM_H
#include <stdint.h>
namespace DUtils {
class Random
{
public:
    static void SeedRand(int seed) { state() = 0x9E3779B97F4A7C15ull ^ (uint64_t)(uint32_t)seed; }
    // uniform in [min, max]
    static int RandomInt(int min, int max)
    {
        uint64_t &s = state();
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return min + (int)((s >> 33) % (uint64_t)(max - min + 1));
    }

private:
    static uint64_t &state()
    {
        static uint64_t s = 0x9E3779B97F4A7C15ull;
        return s;
    }
};
}
#endif
