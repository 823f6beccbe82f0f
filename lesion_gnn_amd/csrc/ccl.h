// The launches of ccl.hip over B images of one size, shared by the one-image entries (ccl.hip)
// and the batch entries (ccl_batch.hip). They check nothing: the entries do.
#pragma once
#include "launch.h"

namespace lgnn_cclk {

bool image_dims_ok(int H, int W);         // H, W > 0 and H * W < 2^31
bool batch_dims_ok(int B, int H, int W);  // and B > 0, B * H * W < 2^31

int launch_label_pool(const float* logits, int B, int K, int Hin, int Win, uint8_t* out, int H,
                      int W, hipStream_t s);
size_t ccl_workspace_bytes(int B, int H, int W);
int launch_ccl(const uint8_t* image, int B, int H, int W, int connectivity, int64_t* labels,
               int32_t* num_labels, int64_t* node_ptr, void* workspace, hipStream_t s);
int launch_ccl_stats(const int64_t* labels, int B, int H, int W, const int64_t* node_ptr,
                     int num_rows, int32_t* stats, double* centroids, int32_t* err, hipStream_t s);

}  // namespace lgnn_cclk
