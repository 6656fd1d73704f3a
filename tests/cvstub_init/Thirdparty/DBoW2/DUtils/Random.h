// stand-in for the reference's Thirdparty/DBoW2/DUtils/Random.h: the members adapter/init/Initializer.cc and its test driver call (same
// names and types) over a seeded 64-bit linear congruential generator, so that a test can repeat the stream.  SeedRandOnce seeds on its
// first call of the process only, as the reference's does; SeedRand always seeds.
#ifndef CVSTUB_DUTILS_RANDOM_H
#define CVSTUB_DUTILS_RANDOM_H
#include <stdint.h>
namespace DUtils {
class Random
{
public:
    static void SeedRand(int seed) { state() = 0x9E3779B97F4A7C15ull ^ (uint64_t)(uint32_t)seed; }
    static void SeedRandOnce(int seed)
    {
        if (!seeded()) { SeedRand(seed); seeded() = true; }
    }
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
    static bool &seeded()
    {
        static bool b = false;
        return b;
    }
};
}
#endif
