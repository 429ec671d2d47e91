// hd_stages_rows.hip -- translation unit of the per-face-row form of the persistent stages: the face-cluster stages of levels 0 / 1
// (hd_face.hpp with HD_FACE_ROWS = 1) and the K-split XCD-local stages of levels 2 / 3 (hd_xcd.hpp with HD_XCD_ROWS = 1) in the graphs of
// hd_sample_rows*, where every face reads its own FiLM rows.  Entry points: hd_stage_api.hpp.
#define HD_FACE_ROWS 1
#define HD_XCD_ROWS 1
#include "hd_face.hpp"

namespace hd {

hipError_t run_face_rows_stage(int C, int own_rows, const FStageP& p, hipStream_t s) {
    if (C == 128 && own_rows == 32) return launch_face_rows_stage<128, 32>(p, s);
    if (C == 256 && own_rows == 32) return launch_face_rows_stage<256, 32>(p, s);
    if (C == 256 && own_rows == 16) return launch_face_rows_stage<256, 16>(p, s);
    return hipErrorInvalidValue;
}

hipError_t run_xcd_rows_stage(int C, const XStageP& p, hipStream_t s) {
    if (C == 1024) return launch_xcd_rows_stage<1024, 4>(p, s);
    if (C == 512) return launch_xcd_rows_stage<512, 16>(p, s);
    return hipErrorInvalidValue;
}

}  // namespace hd
