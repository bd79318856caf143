"""3dinfomax_amd - MI355X-native (gfx950, HIP) implementation of the 3DInfomax pre-training hot path:
PNA(+Net3D)+NT-Xent behind the reference's model_type / model3d_type / loss_func plugin surface.

The package name starts with a digit, so import it with importlib.import_module('3dinfomax_amd') or through
the alias module `infomax3d_amd` at the repository root.
"""
from .graph import (BatchedMolGraph, GraphIndex, NodeDropCollate, laplacian_pos_enc, san_graph, san_laplacian, NoisedCoordinatesCollate, NoisedDistancesCollate, as_batched_graph, batch, bond_graph,  # noqa: F401
                    complete_graph, conformer_collate, contrastive_collate, contrastive_vae_collate, graph_collate,
                    pairwise_distance_collate, GeometricBatch, pytorch_geometric_collate,
                    s_norm_contrastive_collate, s_norm_graph_collate)
from . import synth  # noqa: F401


def __getattr__(name):
    # model / loss classes need torch + the HIP library: import lazily so that the numpy-only parts
    # (synth, graph) stay importable everywhere.
    if name in ('PNA', 'PNAGNN', 'PNALayer', 'PNA_AGGREGATORS', 'PNA_SCALERS'):
        from . import pna
        return getattr(pna, name)
    if name in ('PNAOriginal', 'PNAOriginalSimple', 'PNAGNNOriginal', 'PNAGNNSimple', 'PNATower', 'PNASimpleLayer',
                'MLPReadout'):
        from . import pna_original
        return getattr(pna_original, name)
    if name in ('Net3D', 'Net3DLayer'):
        from . import net3d
        return getattr(net3d, name)
    if name == 'Net3DAE':
        from . import net3d_ae
        return net3d_ae.Net3DAE
    if name in ('NTXent', 'NTXentMultiplePositives', 'NTXentAE', 'NTXentMultiplePositivesSeparate2D', 'NTXentMMDSeparate2D',
                'KLDivergenceMultiplePositives', 'OGBNanLabelBCEWithLogitsLoss', 'OGBNanLabelMSELoss', 'NTXentLocalGlobal',
                'NTXentGlobalLocal', 'NTXentMultiplePositivesV2', 'NTXentMultiplePositivesV3', 'NTXentMinimumMatching',
                'NTXentMaximumSimilarity', 'InfoNCE', 'InfoNCEHard', 'NTXentHard', 'NTXentExtraNegatives', 'NTXentShuffled',
                'BarlowTwinsLoss', 'CosineSimilarityLoss', 'RegularizationLoss', 'CriticLoss', 'NTXentLikelihoodLoss',
                'JSDMultiplePositivesLoss'):
        from . import losses
        return getattr(losses, name)
    if name == 'DistancePredictor':
        from . import distance_predictor
        return distance_predictor.DistancePredictor
    if name in ('OGBGNN', 'GNN_node', 'GNN_node_Virtualnode', 'GINConv'):
        from . import gin
        return getattr(gin, name)
    if name in ('EGNN', 'EGCLayer'):
        from . import egnn
        return getattr(egnn, name)
    if name in ('SAN', 'SAN_NodeLPE', 'GraphTransformerLayer', 'MultiHeadAttentionLayer'):
        from . import san
        return getattr(san, name)
    if name in ('SMP', 'emb', 'init', 'update_e', 'update_v', 'update_u', 'ResidualLayer', 'dist_emb'):      # the reference's class names
        from . import smp
        return getattr(smp, name)
    if name == 'PNALocal':
        from . import pna_local
        return pna_local.PNALocal
    if name in ('GeomolGNNWrapperOGBFeat', 'GeomolGNNOGBFeat', 'GeomolMetaLayer', 'EdgeModel', 'GeomolNodeModel', 'GeomolMLP'):
        from . import geomol
        return getattr(geomol, name)
    if name in ('FCLayer', 'MLP'):
        from . import layers
        return getattr(layers, name)
    if name in ('AtomEncoder', 'BondEncoder'):
        from . import mol_encoder
        return getattr(mol_encoder, name)
    if name in ('PositiveSimilarity', 'NegativeSimilarity', 'ContrastiveAccuracy', 'TrueNegativeRate', 'TruePositiveRate',
                'Uniformity', 'Alignment', 'BatchVariance', 'DimensionCovariance', 'Conformer3DVariance', 'Conformer2DVariance',
                'PositiveProb', 'NegativeProb', 'contrastive_metrics'):
        from . import metrics
        return getattr(metrics, name)
    if name in ('PearsonR', 'Rsquared', 'MAE', 'MeanPredictorLoss', 'QM9DenormalizedL1', 'QM9DenormalizedL2',
                'QM9SingleTargetDenormalizedL1'):
        from . import task_metrics
        return getattr(task_metrics, name)
    if name == 'BYOLwrapper':
        from . import byol
        return byol.BYOLwrapper
    if name == 'Adam':
        from . import optim
        return optim.Adam
    if name in ('set_matmul_precision', 'get_matmul_precision', 'set_fp32_products', 'get_fp32_products'):
        from . import ops
        return getattr(ops, name)
    if name in ('dataset', 'dist', 'tape', 'streams', 'ops', 'net3d_ae', 'pair_head', 'task_metrics', 'gin', 'egnn', 'pna_local', 'geomol', 'byol', 'san', 'smp'):
        import importlib
        return importlib.import_module('.' + name, __name__)
    raise AttributeError(name)


__all__ = ['PNA', 'PNAGNN', 'PNALayer', 'PNA_AGGREGATORS', 'PNA_SCALERS', 'PNAOriginal', 'PNAOriginalSimple',
           'PNAGNNOriginal', 'PNAGNNSimple', 'PNATower', 'PNASimpleLayer', 'MLPReadout', 'Net3D', 'Net3DLayer', 'NTXent',
           'NTXentMultiplePositives', 'FCLayer', 'MLP', 'AtomEncoder', 'BondEncoder', 'contrastive_collate',
           'conformer_collate', 'graph_collate', 's_norm_graph_collate', 's_norm_contrastive_collate', 'BatchedMolGraph', 'batch', 'bond_graph', 'complete_graph', 'Adam', 'PositiveSimilarity',
           'NegativeSimilarity', 'ContrastiveAccuracy', 'TrueNegativeRate', 'TruePositiveRate', 'Uniformity', 'Alignment',
           'BatchVariance', 'DimensionCovariance', 'DistancePredictor', 'pairwise_distance_collate',
           'NodeDropCollate', 'Net3DAE', 'NTXentAE', 'contrastive_vae_collate', 'NTXentMultiplePositivesSeparate2D',
           'NTXentMMDSeparate2D', 'KLDivergenceMultiplePositives', 'Conformer3DVariance', 'Conformer2DVariance',
           'OGBNanLabelBCEWithLogitsLoss', 'OGBNanLabelMSELoss', 'PearsonR', 'Rsquared', 'MAE', 'MeanPredictorLoss',
           'QM9DenormalizedL1', 'QM9DenormalizedL2', 'QM9SingleTargetDenormalizedL1', 'OGBGNN', 'GNN_node',
           'GNN_node_Virtualnode', 'GINConv', 'EGNN', 'EGCLayer', 'PNALocal', 'NTXentLocalGlobal', 'NTXentGlobalLocal',
           'NTXentMultiplePositivesV2', 'NTXentMultiplePositivesV3', 'NTXentMinimumMatching', 'NTXentMaximumSimilarity',
           'GeomolGNNWrapperOGBFeat', 'GeomolGNNOGBFeat', 'GeomolMetaLayer', 'EdgeModel', 'GeomolNodeModel', 'GeomolMLP',
           'InfoNCE', 'InfoNCEHard', 'NTXentHard', 'NTXentExtraNegatives', 'NTXentShuffled', 'BarlowTwinsLoss',
           'CosineSimilarityLoss', 'RegularizationLoss', 'CriticLoss', 'NTXentLikelihoodLoss', 'JSDMultiplePositivesLoss',
           'PositiveProb', 'NegativeProb', 'BYOLwrapper', 'NoisedDistancesCollate', 'NoisedCoordinatesCollate', 'SAN', 'SAN_NodeLPE',
           'GraphTransformerLayer', 'MultiHeadAttentionLayer', 'san_graph', 'laplacian_pos_enc', 'SMP', 'GeometricBatch',
           'pytorch_geometric_collate']
