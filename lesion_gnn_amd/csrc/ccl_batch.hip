// Lesion nodes for a batch of images of one size: the entries over the kernels of ccl.hip with
// their image dimension in use (ccl.h). Reference: src/lesion_gnn/datasets/nodes/lesions.py:150-160
// applied to every image of a batch; the reference takes one image per call.
// Each image's result is what the one-image entry gives for it alone: the class map per image,
// labels numbered from 1 in every image (no component joins two images), statistics in image
// coordinates. The launch counts are those of the one-image entries, whatever B is; node_ptr, the
// exclusive scan of the per-image label counts, is written by the labelling's scan launch and
// places image b's labels at rows node_ptr[b] + l of the batch's flat outputs.
#include "ccl.h"

using namespace lgnn_cclk;

extern "C" int lgnn_label_pool_batch(const float* logits, int batch, int classes, int in_height,
                                     int in_width, uint8_t* out, int height, int width,
                                     void* stream) {
  if (classes < 1 || classes > 255 || !batch_dims_ok(batch, in_height, in_width) ||
      !batch_dims_ok(batch, height, width) || !logits || !out)
    return LGNN_EINVAL;
  return launch_label_pool(logits, batch, classes, in_height, in_width, out, height, width,
                           as_stream(stream));
}

extern "C" size_t lgnn_ccl_batch_workspace_bytes(int batch, int height, int width) {
  return batch_dims_ok(batch, height, width) ? ccl_workspace_bytes(batch, height, width) : 0;
}

extern "C" int lgnn_ccl_batch(const uint8_t* image, int batch, int height, int width,
                              int connectivity, int64_t* labels, int32_t* num_labels,
                              int64_t* node_ptr, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if ((connectivity != 4 && connectivity != 8) || !batch_dims_ok(batch, height, width))
    return LGNN_EINVAL;
  if (!image || !labels || !num_labels || !node_ptr || !workspace ||
      workspace_bytes < lgnn_ccl_batch_workspace_bytes(batch, height, width))
    return LGNN_EINVAL;
  return launch_ccl(image, batch, height, width, connectivity, labels, num_labels, node_ptr,
                    workspace, as_stream(stream));
}

extern "C" int lgnn_ccl_stats_batch(const int64_t* labels, int batch, int height, int width,
                                    const int64_t* node_ptr, int total_nodes, int32_t* stats,
                                    double* centroids, int32_t* err, void* stream) {
  if (!batch_dims_ok(batch, height, width) || total_nodes < 1) return LGNN_EINVAL;
  if (!labels || !node_ptr || !stats || !centroids || !err) return LGNN_EINVAL;
  return launch_ccl_stats(labels, batch, height, width, node_ptr, total_nodes, stats, centroids,
                          err, as_stream(stream));
}
