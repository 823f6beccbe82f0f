"""Node-extractor configs (reference src/lesion_gnn/datasets/nodes) and the lesion-node extraction
from a segmentation output on HIP kernels (lesions.LesionsExtractor.nodes_from_maps and, for a
batch of images, nodes_from_batch; lesions.connected_components_with_stats,
lesions.extract_features_by_cc), and the SIFT-node extraction from an image on HIP kernels
(sift.SiftExtractor.nodes_from_image, nodes_from_batch)."""
