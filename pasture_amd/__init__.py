"""pasture_amd — MI355X-native implementation of pasture's per-point attribute-transform hot path.

Host-side mirror of the reference's interface (pasture-core layout / containers / layout::conversion and the
pasture-algorithms loops) on top of the C ABI in include/pasture_amd.h, which is implemented by hand-written HIP
kernels for gfx950 (pasture_amd/csrc).  No CPU fallback: importing the package without the built extension fails.
"""
from ._capi import PastureError, PasturePanic, product_api, LIB_PATH  # noqa: F401
from .layout import (FieldAlignment, PointAttributeDataType, PointAttributeDefinition, PointAttributeMember, PointLayout,  # noqa: F401
                     attributes)
from .buffers import ExternalColumnsBuffer, ExternalMemoryBuffer, HashMapBuffer, VectorBuffer  # noqa: F401
from .conversion import BufferLayoutConverter, RawPointConverter, Transform  # noqa: F401
from .algorithms import (AABB, calculate_bounds, calculate_bounds_async, compute_centroid, compute_normals, compute_normals_into, minmax_attribute, voxelgrid_filter,  # noqa: F401
                         transform_attribute, Line, Plane, line_inlier_mask, line_inliers, plane_inlier_mask, plane_inliers, ransac_line,
                         ransac_line_fit, ransac_plane, ransac_plane_fit, ransac_sample_indices, OutlierStatistics, knn_search, knn_search_device,
                         outlier_kernel_shape, radius_outlier_mask, remove_radius_outliers, remove_statistical_outliers, statistical_outlier_mask,
                         NO_CLUSTER, cluster_kernel_shape, cluster_mask, euclidean_clusters, extract_clusters, DbscanResult, dbscan,
                         dbscan_kernel_shape, dbscan_phase_times, extract_dbscan_clusters, RegionGrowingResult, extract_regions, region_growing,
                         region_growing_from_knn, region_kernel_shape, region_phase_times, NO_MATCH, NearestNeighbourIndex,
                         cloud_to_cloud_distances, distance_mask, icp, icp_plane, icp_plane_step, icp_step, nearest_neighbours, nearest_neighbours_device, nn_kernel_shape,
                         M3C2Result, m3c2, m3c2_device, m3c2_kernel_shape, m3c2_phase_times, m3c2_work,
                         PmfParameters, classify_ground, extract_ground, grid_dilate, grid_erode, ground_mask, pmf_grid, pmf_kernel_shape, pmf_phase_times,
                         pmf_schedule, remove_ground, classification_mask, hag_kernel_shape, hag_phase_times, height_above_ground,
                         height_above_ground_device, normalize_height, Raster, grid_fill, raster_kernel_shape, raster_phase_times, rasterize,
                         FEATURES, features_kernel_shape, geometric_features, geometric_features_device,
                         poisson_disk_mask, sample_kernel_shape, sample_phase_times, sample_priorities, subsample_min_distance,
                         argsort_attribute, invert_order, morton_order, morton_sort, reorder_kernel_shape, reorder_phase_times, shuffle, shuffle_order,
                         sort_by_attribute, NO_POLYGON, PolygonSet, crop, crop_kernel_shape, overlay, points_in_polygons, polygon_mask,
                         NO_TREE, TreeSegmentation, TreeTops, extract_tree, segment_trees, segment_trees_device, tree_tops, tree_tops_device,
                         trees_kernel_shape, trees_phase_times, trees_work,
                         NO_APEX, SEGMENT_STATS, SegmentTable, segment_planes, segment_statistics, segment_stats_bits, segments_kernel_shape,
                         segments_phase_times,
                         QUANTILE_METHODS, SegmentQuantiles, quantiles_kernel_shape, quantiles_phase_times, rasterize_quantiles, segment_quantiles,
                         NO_NEIGHBOUR, RadiusNeighbours, radius_kernel_shape, radius_neighbour_counts, radius_phase_times, radius_search,
                         radius_search_device)

product_api()  # load libpasture_amd.so now: a missing HIP extension must fail loudly, not at first use
