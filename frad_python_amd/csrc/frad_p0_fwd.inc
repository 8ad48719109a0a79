// frad_p0_fwd.inc -- instantiates k_p0_fwd<FWD_T, LOG2M, LG, MAXT> for LOG2M in [FWD_LO, FWD_HI].
// Included by frad_p0_fwd_*.hip with FWD_T / FWD_NAME / FWD_LO / FWD_HI defined.  FWD_NAME returns 1 = launched, 0 = this
// (log2m, lg) is not built here.
#include "frad_launch.hpp"

namespace frad {
namespace {

template <int LOG2M, int LG>
void fwd_one(const FastCfg& c, dim3 grid, hipStream_t s, const unsigned char* pcm, unsigned char* pay, double* am,
             const Tables& tb, const Geom& g, int ai, int ao) {
    const cx<FWD_T>* tw = static_cast<const cx<FWD_T>*>(tb.tw);
    const cx<FWD_T>* post = static_cast<const cx<FWD_T>*>(tb.post);
    if (c.cg < g.C) {                                 // channel-group kernel (frames larger than a CU's LDS)
        if constexpr (LOG2M >= 8) {
            if (c.threads <= 512) {
                allow_lds(k_p0_fwd_grp<FWD_T, LOG2M, LG, 512>, c.lds);
                hipLaunchKernelGGL((k_p0_fwd_grp<FWD_T, LOG2M, LG, 512>), grid, dim3(c.threads), c.lds, s, pcm, pay, am, tw, post, g);
            } else {
                allow_lds(k_p0_fwd_grp<FWD_T, LOG2M, LG, 1024>, c.lds);
                hipLaunchKernelGGL((k_p0_fwd_grp<FWD_T, LOG2M, LG, 1024>), grid, dim3(c.threads), c.lds, s, pcm, pay, am, tw, post, g);
            }
        }
        return;
    }
#define FRAD_GO(MAXT) do { allow_lds(k_p0_fwd<FWD_T, LOG2M, LG, MAXT>, c.lds); \
        hipLaunchKernelGGL((k_p0_fwd<FWD_T, LOG2M, LG, MAXT>), grid, dim3(c.threads), c.lds, s, pcm, pay, am, tw, post, g, ai, ao); } while (0)
    if (c.threads <= 256) FRAD_GO(256); else if (c.threads <= 512) FRAD_GO(512); else FRAD_GO(1024);
#undef FRAD_GO
}

template <int LOG2M>
int fwd_lg(int lg, const FastCfg& c, dim3 grid, hipStream_t s, const unsigned char* pcm, unsigned char* pay, double* am,
           const Tables& tb, const Geom& g, int ai, int ao) {
    if constexpr (sizeof(FWD_T) == 4) {               // f16 / f32 PCM only
        if (lg == 1) fwd_one<LOG2M, 1>(c, grid, s, pcm, pay, am, tb, g, ai, ao);
        else if (lg == 2) fwd_one<LOG2M, 2>(c, grid, s, pcm, pay, am, tb, g, ai, ao);
        else return 0;
    } else {
        switch (lg) {
            case 0: fwd_one<LOG2M, 0>(c, grid, s, pcm, pay, am, tb, g, ai, ao); break;
            case 1: fwd_one<LOG2M, 1>(c, grid, s, pcm, pay, am, tb, g, ai, ao); break;
            case 2: fwd_one<LOG2M, 2>(c, grid, s, pcm, pay, am, tb, g, ai, ao); break;
            default: fwd_one<LOG2M, 3>(c, grid, s, pcm, pay, am, tb, g, ai, ao); break;
        }
    }
    return 1;
}

}  // namespace

int FWD_NAME(int lg, const FastCfg& c, dim3 grid, hipStream_t s, const unsigned char* pcm, unsigned char* pay, double* am,
             const Tables& tb, const Geom& g, int ai, int ao) {
    switch (c.log2m) {
#define FRAD_CASE(L) case L: if constexpr (L >= FWD_LO && L <= FWD_HI) return fwd_lg<L>(lg, c, grid, s, pcm, pay, am, tb, g, ai, ao); else return 0;
        FRAD_CASE(6) FRAD_CASE(7) FRAD_CASE(8) FRAD_CASE(9) FRAD_CASE(10) FRAD_CASE(11) FRAD_CASE(12) FRAD_CASE(13)
#undef FRAD_CASE
        default: return 0;
    }
}

}  // namespace frad
